"""ops.quant_fp8_div: the one-launch form of the quantization that
Fp8Linear.forward pins (scale = max(amax, 1e-6) / 448, q = e4m3(clamp(x /
scale, +-448))) must be byte-equal to the torch chain it replaces on the GPU:
fp8 bytes, scales, and the linear's output.
"""
import pytest
import torch

from kubeai_amd import ops
from kubeai_amd.engine.quant import FP8_DTYPE, FP8_MAX, Fp8Linear
from kubeai_amd.ops import ref

SHAPES = ((1, 4096), (5, 4096), (48, 4096), (3, 14336))


def _torch_chain(x):
    """Fp8Linear.forward's quantization as it stood before the kernel."""
    a_amax = x.float().abs().amax(dim=-1, keepdim=True).clamp_min(1e-6)
    a_scale = a_amax / FP8_MAX
    xq = (x.float() / a_scale).clamp(-FP8_MAX, FP8_MAX).to(FP8_DTYPE)
    return xq, a_scale


def _rows(T, H, device):
    """randn bf16 with, cycling over the rows from row 1 on: an all-zero row
    (the 1e-6 clamp), a single 3e4 outlier, a row of +-amax only."""
    g = torch.Generator().manual_seed(17 * T + H)
    x = torch.randn(T, H, generator=g)
    for t in range(1, T):
        kind = t % 4
        if kind == 1:
            x[t] = 0.0
        elif kind == 2:
            x[t, (t * 131) % H] = 3e4
        elif kind == 3:
            x[t] = torch.where(x[t] < 0, -2.75, 2.75)
    return x.to(torch.bfloat16).to(device)


def _special_rows(H, device):
    """The three special rows by themselves, for the one-row shape."""
    return _rows(4, H, device)[1:]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_bytes_and_scales_equal_the_torch_chain(shape):
    T, H = shape
    inputs = [_rows(T, H, "cuda")]
    if T < 4:
        # a batch too short for every row kind: each kind as a batch of its own
        inputs += [r.view(1, H).contiguous() for r in _special_rows(H, "cuda")]
    for x in inputs:
        q, scale = ops.quant_fp8_div(x)
        q_ref, scale_ref = _torch_chain(x)
        assert q.dtype == FP8_DTYPE and scale.shape == scale_ref.shape
        assert torch.equal(scale.view(torch.int32), scale_ref.view(torch.int32))
        assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8))


@pytest.mark.gpu
def test_fp8linear_forward_output_unchanged():
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(1024, 4096, generator=g) * 0.02).to(torch.bfloat16).cuda()
    lin = Fp8Linear(w)
    x = _rows(48, 4096, "cuda")
    xq, a_scale = _torch_chain(x)
    want = torch._scaled_mm(
        xq, lin.weight_fp8.t(), scale_a=a_scale, scale_b=lin.weight_scale,
        bias=None, out_dtype=torch.bfloat16,
    )
    got = lin(x)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.gpu
def test_other_inputs_keep_the_torch_chain():
    # 3-D, non-contiguous and fp16 inputs do not take the kernel
    x = _rows(6, 4096, "cuda")
    for y in (x.view(2, 3, 4096), x[:, ::2], x.to(torch.float16)):
        q, scale = ops.quant_fp8_div(y)
        q_ref, scale_ref = _torch_chain(y)
        assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8))
        assert torch.equal(scale, scale_ref)


def test_cpu_is_the_torch_chain():
    x = _rows(5, 4096, "cpu")
    q, scale = ops.quant_fp8_div(x)
    q_ref, scale_ref = _torch_chain(x)
    assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8))
    assert torch.equal(scale, scale_ref)
    q2, scale2 = ref.quant_fp8_div(x)
    assert torch.equal(q2.view(torch.uint8), q_ref.view(torch.uint8))
    assert torch.equal(scale2, scale_ref)
