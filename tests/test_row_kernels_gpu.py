"""The eleven row kernels (csrc/row_kernels.hip, csrc/activation.hip) against
the fp64 oracles of row_oracle.py, whose bounds are derived there and whose
power to reject a subtly wrong kernel is shown on the CPU by
test_row_oracle.py.

Inputs are made on the CPU and copied over, `_C.*` is called with outputs the
caller allocated, and everything is copied back and checked on the CPU. No
expected value comes from ops/ref.py. Every tensor a kernel sees is the middle
of a buffer with one sentinel row above and one below: a stray store at a
ragged tail shows as a changed sentinel, not as a fault.
"""
import math

import pytest
import torch

import row_oracle as ro

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _c():
    from kubeai_amd import _C

    return _C


def _bits(t):
    return t.contiguous().view(torch.uint8)


class Guarded:
    """Device tensors between sentinel rows, by name."""

    def __init__(self):
        self.bufs = {}

    def put(self, name, t):
        """Copy CPU tensor t (rows along dim 0) over; returns the device
        view a kernel gets."""
        rows = t.shape[0]
        shape = (rows + 2,) + tuple(t.shape[1:])
        buf = torch.full((math.prod(shape) * t.element_size(),), SENTINEL,
                         dtype=torch.uint8).view(t.dtype).view(shape)
        buf[1:rows + 1] = t
        dev = buf.cuda()
        self.bufs[name] = (dev, rows)
        return dev[1:rows + 1]

    def empty(self, name, shape, dtype):
        """An output: filled with another pattern, so that an element the
        kernel never wrote cannot pass for a result."""
        n_bytes = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        t = torch.full((n_bytes,), 0x5A, dtype=torch.uint8).view(dtype)
        return self.put(name, t.view(shape))

    def fetch(self, name):
        """The CPU copy of the middle rows; the sentinels must be intact."""
        dev, rows = self.bufs[name]
        host = dev.cpu()
        for edge in (host[:1], host[rows + 1:]):
            assert bool((_bits(edge) == SENTINEL).all()), (
                f"{name}: sentinel row overwritten")
        return host[1:rows + 1].contiguous()

    def unchanged(self, name, t):
        got = self.fetch(name).view(t.shape)
        assert torch.equal(_bits(got), _bits(t)), f"{name} was modified"


def _torch_chain(y):
    """Fp8Linear.forward's quantization, torch ops on the device of y."""
    amax = y.float().abs().amax(dim=-1, keepdim=True).clamp_min(1e-6)
    scale = amax / 448.0
    q = (y.float() / scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale.view(-1)


def run(kernel, inp):
    """One guarded call of `_C.<kernel>` -> CPU outputs as row_oracle.verify
    names them. Asserts the side effects: sentinels, untouched inputs."""
    C, g = _c(), Guarded()
    out = {}
    if kernel in ro.ACT_KERNELS or kernel in ro.MAX_KERNELS:
        x = g.put("x", inp["x"])
        T = x.shape[0]
        W = x.shape[1] // (2 if kernel in ro.GATED else 1)
        if kernel in ro.ACT_KERNELS:
            getattr(C, kernel)(g.empty("y", (T, W), torch.bfloat16), x)
            out["y"] = g.fetch("y")
        else:
            getattr(C, kernel)(g.empty("q", (T, W), torch.uint8),
                               g.empty("scale", (T,), torch.float32), x)
            out["q"], out["scale"] = g.fetch("q"), g.fetch("scale")
        g.unchanged("x", inp["x"])
        return out

    w, eps = g.put("w", inp["w"].view(1, -1))[0], inp["eps"]
    if kernel == "embed_rmsnorm_fp8":
        table, ids = g.put("table", inp["table"]), g.put("ids", inp["ids"])
        T, H = ids.shape[0], table.shape[1]
        C.embed_rmsnorm_fp8(g.empty("q", (T, H), torch.uint8),
                            g.empty("scale", (T,), torch.float32),
                            g.empty("x_out", (T, H), torch.bfloat16),
                            ids, table, w, eps)
        g.unchanged("table", inp["table"])
        g.unchanged("ids", inp["ids"])
        out["x_out"] = g.fetch("x_out")
    else:
        x = g.put("x", inp["x"])
        T, H = x.shape
        if kernel == "rmsnorm":
            C.rmsnorm(g.empty("y", (T, H), torch.bfloat16), x, w, eps)
            out["y"] = g.fetch("y")
            g.unchanged("x", inp["x"])
        elif kernel == "fused_add_rmsnorm":
            C.fused_add_rmsnorm(x, g.put("r", inp["r"]), w, eps)
            out["y"], out["residual"] = g.fetch("x"), g.fetch("r")
        else:
            q = g.empty("q", (T, H), torch.uint8)
            scale = g.empty("scale", (T,), torch.float32)
            if kernel == "rmsnorm_fp8":
                C.rmsnorm_fp8(q, scale, x, w, eps)
                g.unchanged("x", inp["x"])
            elif kernel == "fused_add_rmsnorm_fp8":
                C.fused_add_rmsnorm_fp8(q, scale, x, g.put("r", inp["r"]), w,
                                        eps)
                g.unchanged("x", inp["x"])
                out["residual"] = g.fetch("r")
            else:
                # write_rows=False first: x and residual are only read
                r = g.put("r", inp["r"])
                C.fused_add_rmsnorm_fp8_div(q, scale, x, r, w, eps, False)
                g.unchanged("x", inp["x"])
                g.unchanged("r", inp["r"])
                q_ro, scale_ro = g.fetch("q"), g.fetch("scale")
                q2 = g.empty("q2", (T, H), torch.uint8)
                scale2 = g.empty("scale2", (T,), torch.float32)
                C.fused_add_rmsnorm_fp8_div(q2, scale2, x, r, w, eps, True)
                out["y"], out["residual"] = g.fetch("x"), g.fetch("r")
                assert torch.equal(g.fetch("q2"), q_ro)
                assert torch.equal(_bits(g.fetch("scale2")), _bits(scale_ro))
                # the torch chain on the row the kernel left in x
                q_t, scale_t = _torch_chain(x)
                assert torch.equal(q_t.cpu(), q_ro)
                assert torch.equal(_bits(scale_t.cpu()), _bits(scale_ro))
    if "q" in g.bufs:
        out["q"], out["scale"] = g.fetch("q"), g.fetch("scale")
    g.unchanged("w", inp["w"])
    return out


def _n_rows(inp):
    return (inp["ids"] if "ids" in inp else inp["x"]).shape[0]


@pytest.mark.parametrize("H", ro.WIDTHS)
@pytest.mark.parametrize("kernel", ro.KERNELS)
def test_kernel_against_fp64_oracle(kernel, H):
    """Every family at T = 3 (the needle family: one row per needle
    position), then T = 1: a row must not depend on its neighbours, so the
    one-row call on row t equals row t of the batch bit for bit."""
    for family in ro.families(kernel):
        inp = ro.make_inputs(kernel, family, 3, H)
        out = run(kernel, inp)
        results = ro.verify(kernel, inp, out)
        for r in results:
            print(f"ROW_GPU {kernel} H={H} {family} {r}")
        assert not ro.failures(results), (kernel, H, family)
        n = _n_rows(inp)
        for t in sorted({0, 1, n // 2, n - 1}):
            one = run(kernel, ro.row_slice(kernel, inp, t))
            for name, got in one.items():
                assert torch.equal(_bits(got), _bits(out[name][t:t + 1])), (
                    kernel, H, family, f"row {t} of {name} depends on the batch")
    torch.cuda.synchronize()


def test_quant_fp8_div_equals_the_torch_chain():
    """The existing byte equality, at the widths of this file."""
    for H in ro.WIDTHS:
        for family in ro.families("quant_fp8_div"):
            inp = ro.make_inputs("quant_fp8_div", family, 3, H)
            out = run("quant_fp8_div", inp)
            q_t, scale_t = _torch_chain(inp["x"].cuda())
            assert torch.equal(q_t.cpu(), out["q"]), (H, family)
            assert torch.equal(_bits(scale_t.cpu()), _bits(out["scale"]))


# ---------------------------------------------------------------------------
# host contract: a bad argument raises before any launch, T = 0 launches
# nothing
# ---------------------------------------------------------------------------

H0 = 264


def _args(kernel, T=2, H=H0):
    """Valid device arguments of `_C.<kernel>` by name, in call order."""
    bf16 = dict(dtype=torch.bfloat16, device="cuda")
    a = {}
    if kernel in ro.NORM_KERNELS and kernel not in ("rmsnorm",
                                                    "fused_add_rmsnorm"):
        a["out"] = torch.zeros(T, H, dtype=torch.uint8, device="cuda")
        a["out_scale"] = torch.zeros(T, dtype=torch.float32, device="cuda")
    elif kernel in ro.MAX_KERNELS:
        a["out"] = torch.zeros(T, H, dtype=torch.uint8, device="cuda")
        a["out_scale"] = torch.zeros(T, dtype=torch.float32, device="cuda")
    elif kernel == "rmsnorm":
        a["out"] = torch.zeros(T, H, **bf16)
    if kernel == "embed_rmsnorm_fp8":
        a["x_out"] = torch.zeros(T, H, **bf16)
        a["ids"] = torch.zeros(T, dtype=torch.int32, device="cuda")
        a["table"] = torch.ones(4, H, **bf16)
    else:
        width = 2 * H if kernel in ro.GATED else H
        a["x"] = torch.ones(T, width, **bf16)
    if kernel in ro.FUSED:
        a["residual"] = torch.ones(T, H, **bf16)
    if kernel in ro.NORM_KERNELS:
        a["weight"] = torch.ones(H, **bf16)
        a["eps"] = 1e-5
    if kernel == "fused_add_rmsnorm_fp8_div":
        a["write_rows"] = True
    return a


ROW_KERNELS_HIP = ro.NORM_KERNELS + ro.MAX_KERNELS


def _violations(kernel):
    """name -> (argument, replacement) that launch_* must refuse."""
    dev = dict(device="cuda")
    v = {}
    if kernel in ro.NORM_KERNELS:
        v["weight_short"] = ("weight", torch.ones(H0 - 8, dtype=torch.bfloat16, **dev))
        v["weight_long"] = ("weight", torch.ones(H0 + 8, dtype=torch.bfloat16, **dev))
        v["weight_fp32"] = ("weight", torch.ones(H0, dtype=torch.float32, **dev))
        v["weight_strided"] = (
            "weight", torch.ones(2 * H0, dtype=torch.bfloat16, **dev)[::2])
        v["weight_2d_wrong"] = (
            "weight", torch.ones(2, H0, dtype=torch.bfloat16, **dev))
    if kernel == "rmsnorm":
        v["out_short"] = ("out", torch.zeros(1, H0, dtype=torch.bfloat16, **dev))
        v["out_fp32"] = ("out", torch.zeros(2, H0, dtype=torch.float32, **dev))
    if kernel in ro.FUSED:
        v["residual_short"] = (
            "residual", torch.ones(1, H0, dtype=torch.bfloat16, **dev))
        v["residual_fp16"] = (
            "residual", torch.ones(2, H0, dtype=torch.float16, **dev))
    if "out_scale" in _args(kernel):
        v["out_short"] = ("out", torch.zeros(1, H0, dtype=torch.uint8, **dev))
        v["out_two_bytes"] = ("out", torch.zeros(2, H0, dtype=torch.bfloat16, **dev))
        v["out_strided"] = (
            "out", torch.zeros(2, 2 * H0, dtype=torch.uint8, **dev)[:, ::2])
        v["scale_short"] = ("out_scale", torch.zeros(1, dtype=torch.float32, **dev))
        v["scale_fp64"] = ("out_scale", torch.zeros(2, dtype=torch.float64, **dev))
        v["scale_fp16"] = ("out_scale", torch.zeros(2, dtype=torch.float16, **dev))
    if kernel == "embed_rmsnorm_fp8":
        v["x_out_short"] = ("x_out", torch.zeros(1, H0, dtype=torch.bfloat16, **dev))
        v["ids_int64"] = ("ids", torch.zeros(2, dtype=torch.int64, **dev))
    else:
        width = 2 * H0 if kernel in ro.GATED else H0
        v["x_fp16"] = ("x", torch.ones(2, width, dtype=torch.float16, **dev))
        v["x_strided"] = (
            "x", torch.ones(2, 2 * width, dtype=torch.bfloat16, **dev)[:, ::2])
        v["x_width_not_8"] = (
            "x", torch.ones(2, width + 4, dtype=torch.bfloat16, **dev))
    return v


@pytest.mark.parametrize("kernel", ROW_KERNELS_HIP)
def test_bad_arguments_raise(kernel):
    fn = getattr(_c(), kernel)
    fn(*_args(kernel).values())  # the valid call passes
    for name, (arg, bad) in _violations(kernel).items():
        args = _args(kernel)
        assert arg in args, (kernel, name)
        args[arg] = bad
        with pytest.raises(RuntimeError):
            fn(*args.values())
    torch.cuda.synchronize()


@pytest.mark.parametrize("kernel", ROW_KERNELS_HIP)
def test_zero_rows_launch_nothing(kernel):
    fn = getattr(_c(), kernel)
    args = _args(kernel, T=0)
    fn(*args.values())  # an empty grid would raise
    torch.cuda.synchronize()
    # and the arguments are still validated
    if kernel in ro.NORM_KERNELS:
        args["weight"] = torch.ones(H0 + 8, dtype=torch.bfloat16, device="cuda")
        with pytest.raises(RuntimeError):
            fn(*args.values())
