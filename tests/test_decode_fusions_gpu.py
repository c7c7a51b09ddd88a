"""Decode-layer small kernels: the register-resident row kernels at every
iteration-count / block-width path, and the two fused launches
(rope + KV-cache write, flash-decoding merge + fp8 quant) bit-for-bit
against the unfused kernel sequences they replace.
"""
import math

import pytest
import torch

import kubeai_amd.ops as ops
from kubeai_amd.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda"

# 264 = 33 vectors (one iteration, ragged tail); 4104 = 513 vectors (3
# iterations, ragged); 16384 = the 8-iteration boundary of the 256 block
# (rmsnorm family; quant_fp8 runs it as 512 threads x 4)
ROW_H = [264, 4104, 4096, 16384]
# 32768: 512 threads x 8, the width limit of the whole family
# (row_kernels.hip)
ROW_H_FP8 = ROW_H + [32768]
ROW_T = [1, 3]


def assert_close_bf16(out, ref_f32, atol=2e-2, rtol=2e-2):
    ref_bf16 = ref_f32.to(torch.bfloat16).float()
    torch.testing.assert_close(out.float(), ref_bf16, atol=atol, rtol=rtol)


def _dequant(q8, scale):
    return q8.float() * scale.view(-1, 1)


def _bytes(t):
    return t.view(torch.uint8) if t.dtype != torch.bfloat16 else t.view(torch.int16)


@pytest.fixture(autouse=True)
def _seed():
    torch.manual_seed(4321)


# ---------------------------------------------------------------- row kernels


@pytest.mark.parametrize("H", ROW_H_FP8)
@pytest.mark.parametrize("T", ROW_T)
def test_rmsnorm_rows(T, H):
    x = torch.randn(T, H, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(H, dtype=torch.bfloat16, device=DEV)
    out = ops.rmsnorm(x, w, 1e-5)
    assert_close_bf16(out, ref.rmsnorm(x.float(), w.float(), 1e-5))


@pytest.mark.parametrize("H", ROW_H_FP8)
@pytest.mark.parametrize("T", ROW_T)
def test_fused_add_rmsnorm_rows(T, H):
    x = torch.randn(T, H, dtype=torch.bfloat16, device=DEV)
    res = torch.randn(T, H, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(H, dtype=torch.bfloat16, device=DEV)
    y_ref, _ = ref.fused_add_rmsnorm(x.float(), res.float(), w.float(), 1e-5)
    res_bf16 = (x.float() + res.float()).to(torch.bfloat16)
    y, res_out = ops.fused_add_rmsnorm(x.clone(), res.clone(), w, 1e-5)
    assert torch.equal(res_out, res_bf16)
    assert_close_bf16(y, y_ref, atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("H", ROW_H_FP8)
@pytest.mark.parametrize("T", ROW_T)
def test_rmsnorm_fp8_rows(T, H):
    x = torch.randn(T, H, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(H, dtype=torch.bfloat16, device=DEV)
    q8, scale = ops.rmsnorm_fp8(x, w, 1e-5)
    expected = ref.rmsnorm(x.float(), w.float(), 1e-5)
    torch.testing.assert_close(
        scale, expected.abs().amax(dim=-1) / 448.0, atol=1e-2, rtol=1e-2
    )
    torch.testing.assert_close(_dequant(q8, scale), expected, atol=0.07, rtol=0.07)


@pytest.mark.parametrize("H", ROW_H_FP8)
@pytest.mark.parametrize("T", ROW_T)
def test_fused_add_rmsnorm_fp8_rows(T, H):
    x = torch.randn(T, H, dtype=torch.bfloat16, device=DEV)
    res = torch.randn(T, H, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(H, dtype=torch.bfloat16, device=DEV)
    y_ref, _ = ref.fused_add_rmsnorm(x.float(), res.float(), w.float(), 1e-5)
    res_bf16 = (x.float() + res.float()).to(torch.bfloat16)
    q8, scale = ops.fused_add_rmsnorm_fp8(x, res, w, 1e-5)
    assert torch.equal(res, res_bf16)  # updated in place
    torch.testing.assert_close(_dequant(q8, scale), y_ref, atol=0.07, rtol=0.07)


@pytest.mark.parametrize("H", ROW_H_FP8)
@pytest.mark.parametrize("T", ROW_T)
def test_quant_fp8_rows(T, H):
    x = torch.randn(T, H, dtype=torch.bfloat16, device=DEV) * 3
    q8, scale = ops.quant_fp8(x)
    # scale == amax/448 within 1 ulp
    want = x.float().abs().amax(-1).clamp_min(1e-6) / 448
    inf = torch.full_like(want, float("inf"))
    assert bool(
        ((scale >= torch.nextafter(want, -inf)) & (scale <= torch.nextafter(want, inf))).all()
    ), (scale, want)
    torch.testing.assert_close(_dequant(q8, scale), x.float(), atol=0.1, rtol=0.07)
    # matches torch's cast given the same scale
    expected_q = (x.float() / scale.view(-1, 1)).clamp(-448, 448).to(
        torch.float8_e4m3fn
    )
    assert (q8.view(torch.uint8) == expected_q.view(torch.uint8)).float().mean() > 0.99


# 264: one ragged iteration; 14336: llama-3-8b (512 threads x 4 iterations,
# ragged); 28672: llama-3-70b (512 x 8, ragged)
@pytest.mark.parametrize("I", [264, 14336, 28672])
@pytest.mark.parametrize("T", ROW_T)
def test_silu_and_mul_fp8_rows(T, I):
    x = torch.randn(T, 2 * I, dtype=torch.bfloat16, device=DEV)
    q8, scale = ops.silu_and_mul_fp8(x)
    expected = ref.silu_and_mul(x.float())
    torch.testing.assert_close(_dequant(q8, scale), expected, atol=0.07, rtol=0.07)


# The fused and unfused norms are one kernel template, and x + 0.0f is exact
# (randn bf16 has no exact zeros in practice, the only place a sign could
# differ): adding a zero residual must not change a single output bit.
@pytest.mark.parametrize("H", [264, 4104, 16384, 32768])
@pytest.mark.parametrize("T", ROW_T)
def test_rmsnorm_shared_load_phase(T, H):
    x = torch.randn(T, H, dtype=torch.bfloat16, device=DEV)
    w = torch.randn(H, dtype=torch.bfloat16, device=DEV)
    zeros = torch.zeros_like(x)

    y, res = ops.fused_add_rmsnorm(x.clone(), zeros.clone(), w, 1e-5)
    assert torch.equal(ops.rmsnorm(x, w, 1e-5), y)
    assert torch.equal(res, x)

    q8, scale = ops.rmsnorm_fp8(x, w, 1e-5)
    res = zeros.clone()
    q8_f, scale_f = ops.fused_add_rmsnorm_fp8(x.clone(), res, w, 1e-5)
    assert torch.equal(_bytes(q8_f), _bytes(q8))
    assert torch.equal(scale_f, scale)
    assert torch.equal(res, x)


# 264: ragged grid (33 vectors per row); 14336: llama-3-8b; T = 300 at
# I = 14336 is 537600 vectors, beyond the 2048 x 256 threads of the capped
# grid, so the grid-stride loop takes a second trip
@pytest.mark.parametrize("op", ["silu_and_mul", "gelu_and_mul"])
@pytest.mark.parametrize("T,I", [(1, 264), (3, 264), (1, 14336), (3, 14336), (300, 14336)])
def test_act_and_mul_rows(op, T, I):
    x = torch.randn(T, 2 * I, dtype=torch.bfloat16, device=DEV)
    out = getattr(ops, op)(x)
    assert out.shape == (T, I) and out.dtype == torch.bfloat16
    assert_close_bf16(out, getattr(ref, op)(x.float()))


# ------------------------------------------------------------ rope_and_cache


@pytest.mark.parametrize("cache_dtype", [torch.bfloat16, torch.float8_e5m2])
@pytest.mark.parametrize("layout", ["qkv_views", "separate"])
@pytest.mark.parametrize("nq,nkv,hd", [(32, 8, 128), (8, 1, 128), (8, 4, 256)])
def test_rope_and_cache_equals_unfused(nq, nkv, hd, layout, cache_dtype):
    T, nb, bs = 5, 4, 16
    qkv = torch.randn(T, (nq + 2 * nkv) * hd, dtype=torch.bfloat16, device=DEV)
    pos = torch.randint(0, 4000, (T,), dtype=torch.int32, device=DEV)
    cs = ref.make_cos_sin_cache(hd, 4096, 500000.0).to(DEV)
    slots = torch.randperm(nb * bs, device=DEV)[:T].to(torch.int64)
    slots[2] = -1  # pad row: rotated, not cached
    kc0 = torch.randn(nb, nkv, bs, hd, device=DEV).to(cache_dtype)
    vc0 = torch.randn(nb, nkv, bs, hd, device=DEV).to(cache_dtype)

    def split(buf):
        q, k, v = buf.split([nq * hd, nkv * hd, nkv * hd], dim=-1)
        q = q.unflatten(-1, (nq, hd))
        k = k.unflatten(-1, (nkv, hd))
        v = v.unflatten(-1, (nkv, hd))
        if layout == "separate":
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        return q, k, v

    q_a, k_a, v_a = split(qkv.clone())
    kc_a, vc_a = kc0.clone(), vc0.clone()
    ops.rope(q_a, k_a, pos, cs)
    ops.reshape_and_cache(k_a, v_a, kc_a, vc_a, slots)

    q_b, k_b, v_b = split(qkv.clone())
    kc_b, vc_b = kc0.clone(), vc0.clone()
    q_r, k_r = ops.rope_and_cache(q_b, k_b, v_b, pos, cs, kc_b, vc_b, slots)

    assert q_r.data_ptr() == q_b.data_ptr() and k_r.data_ptr() == k_b.data_ptr()
    assert torch.equal(q_b, q_a)
    assert torch.equal(k_b, k_a)
    assert torch.equal(v_b, v_a)
    assert torch.equal(_bytes(kc_b), _bytes(kc_a))
    assert torch.equal(_bytes(vc_b), _bytes(vc_a))
    # the caches did change (the comparison is not of two untouched clones)
    assert not torch.equal(_bytes(kc_b), _bytes(kc0))


# ------------------------------------------------------- merge + fp8 quant


def _decode_case(nq, nkv, hd, lens):
    bs = 16
    B = len(lens)
    max_blocks = max((L + bs - 1) // bs for L in lens)
    nb = B * max_blocks + 1
    kc = torch.randn(nb, nkv, bs, hd, dtype=torch.bfloat16, device=DEV)
    vc = torch.randn(nb, nkv, bs, hd, dtype=torch.bfloat16, device=DEV)
    bt = torch.arange(1, nb, dtype=torch.int32, device=DEV).reshape(B, max_blocks)
    seq_lens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    q = torch.randn(B, nq, hd, dtype=torch.bfloat16, device=DEV)
    return q, kc, vc, bt, seq_lens, 1.0 / math.sqrt(hd)


def _check_fp8_out(nq, nkv, hd, lens, window=0):
    q, kc, vc, bt, seq_lens, scale = _decode_case(nq, nkv, hd, lens)
    B = len(lens)
    out_a = ops.paged_attention_decode(q, kc, vc, bt, seq_lens, scale, window=window)
    f8_a, sc_a = ops.quant_fp8(out_a.view(B, -1))
    out_b, f8_b, sc_b = ops.paged_attention_decode(
        q, kc, vc, bt, seq_lens, scale, window=window, fp8_out=True
    )
    assert f8_b.shape == (B, nq * hd) and sc_b.shape == (B,)
    assert torch.equal(out_b, out_a)
    assert torch.equal(f8_b.view(torch.uint8), f8_a.view(torch.uint8))
    assert torch.equal(sc_b, sc_a)


@pytest.mark.parametrize("nq,nkv,hd", [(32, 8, 128), (8, 4, 256)])
@pytest.mark.parametrize("lens", [[1], [30, 7], [257, 64, 19, 100]])
def test_decode_fp8_out_equals_unfused(nq, nkv, hd, lens):
    _check_fp8_out(nq, nkv, hd, lens)


def test_decode_fp8_out_window():
    _check_fp8_out(32, 8, 128, [100, 37], window=48)


def test_decode_fp8_out_single_split_fallback():
    # B * n_kv = 2048 workgroups: the host picks n_splits == 1, there is no
    # merge launch, and the wrapper quantizes `out` with quant_fp8
    _check_fp8_out(32, 8, 128, [17] * 256)
