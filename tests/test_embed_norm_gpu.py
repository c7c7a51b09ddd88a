"""The two row ops at the ends of the decoder stack against the op sequences
they replace, byte for byte.

embed_rmsnorm_fp8(ids, table, w, eps)   == embedding -> rmsnorm_fp8
fused_add_rmsnorm_fp8_div(x, r, w, eps) == fused_add_rmsnorm -> quant_fp8_div

Shapes: H = 256 is one vector per thread with most of the block idle, H =
4096 two per thread (the llama-3-8b row); T = 1, 5 and 48 rows. The ids hold
0, V - 1 and repeats; the rows of the second op a plain randn row, an
all-zero row (scale clamp) and a row with a 3e4 outlier (saturating bytes).
"""
import pytest
import torch

import kubeai_amd.ops as ops
from kubeai_amd.ops import ref

gpu = pytest.mark.gpu
EPS = 1e-5
V = 1000


def _ids(T, gen):
    ids = torch.randint(0, V, (T,), generator=gen, dtype=torch.int32)
    fixed = [0, V - 1, 7, 7, V - 1]
    for i, t in enumerate(fixed[:T]):
        ids[(i * 3) % T if T > 1 else 0] = t
    return ids


@gpu
@pytest.mark.parametrize("H", [256, 4096])
@pytest.mark.parametrize("T", [1, 5, 48])
def test_embed_rmsnorm_fp8_equals_two_ops(T, H):
    gen = torch.Generator().manual_seed(1000 * T + H)
    table = torch.randn(V, H, generator=gen).to(torch.bfloat16).cuda()
    w = (1.0 + 0.1 * torch.randn(H, generator=gen)).to(torch.bfloat16).cuda()
    ids = _ids(T, gen).cuda()
    if T >= 5:
        assert {0, V - 1} <= set(ids.tolist())
        assert len(set(ids.tolist())) < T  # repeats

    x_ref = torch.nn.functional.embedding(ids.long(), table)
    q_ref, s_ref = ops.rmsnorm_fp8(x_ref, w, EPS)

    table0 = table.clone()
    x, q, s = ops.embed_rmsnorm_fp8(ids, table, w, EPS)
    assert x.shape == (T, H) and x.dtype == torch.bfloat16
    assert q.shape == (T, H) and s.shape == (T,)
    assert torch.equal(x.view(torch.int16), x_ref.view(torch.int16))
    assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8))
    assert torch.equal(s, s_ref)
    assert torch.equal(table.view(torch.int16), table0.view(torch.int16))


@gpu
def test_embed_ids_are_clamped_into_the_table():
    gen = torch.Generator().manual_seed(3)
    H = 256
    table = torch.randn(V, H, generator=gen).to(torch.bfloat16).cuda()
    w = torch.ones(H, dtype=torch.bfloat16).cuda()
    bad = torch.tensor([-5, V, 2**31 - 1, 3], dtype=torch.int32).cuda()
    good = torch.tensor([0, V - 1, V - 1, 3], dtype=torch.int32).cuda()
    a = ops.embed_rmsnorm_fp8(bad, table, w, EPS)
    b = ops.embed_rmsnorm_fp8(good, table, w, EPS)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
    assert torch.equal(a[1].view(torch.uint8), b[1].view(torch.uint8))
    assert torch.equal(a[2], b[2])


@gpu
def test_embed_int64_ids_take_the_two_op_path():
    gen = torch.Generator().manual_seed(4)
    H = 256
    table = torch.randn(V, H, generator=gen).to(torch.bfloat16).cuda()
    w = torch.ones(H, dtype=torch.bfloat16).cuda()
    ids = _ids(5, gen).cuda()
    a = ops.embed_rmsnorm_fp8(ids.long(), table, w, EPS)
    b = ops.embed_rmsnorm_fp8(ids, table, w, EPS)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
    assert torch.equal(a[1].view(torch.uint8), b[1].view(torch.uint8))
    assert torch.equal(a[2], b[2])


def _final_norm_inputs(T, H, gen):
    x = torch.randn(T, H, generator=gen)
    r = torch.randn(T, H, generator=gen)
    if T >= 5:
        x[1] = 0.0
        r[1] = 0.0  # all-zero row: amax clamps at 1e-6
        x[3, 17] = 3e4  # outlier: the rest of the row rounds to small bytes
    w = 1.0 + 0.1 * torch.randn(H, generator=gen)
    return (t.to(torch.bfloat16).cuda() for t in (x, r, w))


@gpu
@pytest.mark.parametrize("write_rows", [False, True])
@pytest.mark.parametrize("T", [1, 5, 48])
def test_final_norm_quant_equals_two_ops(T, write_rows):
    H = 4096
    x, r, w = _final_norm_inputs(T, H, torch.Generator().manual_seed(50 + T))
    x_ref, r_ref = x.clone(), r.clone()
    ops.fused_add_rmsnorm(x_ref, r_ref, w, EPS)  # in place
    q_ref, s_ref = ops.quant_fp8_div(x_ref)

    x0, r0 = x.clone(), r.clone()
    q, s = ops.fused_add_rmsnorm_fp8_div(x, r, w, EPS, write_rows=write_rows)
    assert q.shape == (T, H) and q.dtype == torch.float8_e4m3fn
    assert s.shape == s_ref.shape == (T, 1) and s.stride() == s_ref.stride()
    assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8))
    assert torch.equal(s, s_ref)
    if T >= 5:
        assert float(s[1]) == pytest.approx(1e-6 / 448.0, rel=1e-6)
    # the rows: updated as fused_add_rmsnorm updates them, or only read
    want_x, want_r = (x_ref, r_ref) if write_rows else (x0, r0)
    assert torch.equal(x.view(torch.int16), want_x.view(torch.int16))
    assert torch.equal(r.view(torch.int16), want_r.view(torch.int16))


# ---- fallbacks (no GPU) ----------------------------------------------------
def test_embed_rmsnorm_fp8_cpu_fallback():
    gen = torch.Generator().manual_seed(1)
    table = torch.randn(V, 64, generator=gen).to(torch.bfloat16)
    w = (1.0 + 0.1 * torch.randn(64, generator=gen)).to(torch.bfloat16)
    ids = _ids(5, gen)
    x, q, s = ops.embed_rmsnorm_fp8(ids, table, w, EPS)
    x_ref = table[ids.long()]
    q_ref, s_ref = ref.quant_fp8(ref.rmsnorm(x_ref, w, EPS))
    assert torch.equal(x, x_ref)
    assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8))
    assert torch.equal(s, s_ref)


def test_fused_add_rmsnorm_fp8_div_cpu_fallback():
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(5, 64, generator=gen).to(torch.bfloat16)
    r = torch.randn(5, 64, generator=gen).to(torch.bfloat16)
    w = (1.0 + 0.1 * torch.randn(64, generator=gen)).to(torch.bfloat16)
    y_ref, _ = ref.fused_add_rmsnorm(x, r, w, EPS)
    q_ref, s_ref = ref.quant_fp8_div(y_ref)
    q, s = ops.fused_add_rmsnorm_fp8_div(x.clone(), r.clone(), w, EPS)
    assert s.shape == (5, 1)
    assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8))
    assert torch.equal(s, s_ref)
