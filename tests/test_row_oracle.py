"""CPU self-check of the row-kernel checker (row_oracle.py).

test_row_kernels_gpu.py trusts the fp64 oracles, the derived bounds and the
input families. Here fp32 emulations of the eleven kernels in plain torch
(torch's own summation order, not the kernels') stand in for the GPU:

* the unmutated emulation must PASS every check on every family at all eight
  widths, the 99.5 % exact-byte cap included;
* every mutant of MUTANTS must FAIL on its named family, at every width it
  changes anything at.

Run with -s to see each figure.
"""
import pytest
import torch

import row_oracle as ro

# ---------------------------------------------------------------------------
# fp32 emulations
# ---------------------------------------------------------------------------


def _bf16(y32, mut):
    if mut == "bf16_truncated":
        bits = y32.contiguous().view(torch.int32) & -65536
        return bits.view(torch.float32).bfloat16()
    return y32.bfloat16()


def _e4m3_bytes(t32, mut):
    t = t32.clamp(-ro.FP8_MAX, ro.FP8_MAX)
    if mut == "fp8_truncated":
        st = ro.step_e4m3(t.double()).float()
        t = torch.trunc(t / st) * st
    return t.to(ro.FP8).view(torch.uint8)


def _quant(y32, form, mut, amax_of=None):
    """common.h::row_scale_fp8 + quant8_fp8 (form "mul") or their _div
    forms, on fp32 rows."""
    a = (y32 if amax_of is None else amax_of).abs()
    if mut == "amax_misses_last_vector":
        a = torch.cat([a[:, :-8], torch.zeros_like(a[:, :1])], dim=1)
    amax = a.amax(-1)
    if mut != "clamp_missing":
        amax = torch.maximum(amax, ro.CLAMP_F32)
    top = torch.tensor(240.0 if mut == "scale_amax_over_240" else ro.FP8_MAX)
    if form == "mul":
        scale = amax / top
        t = y32 * (top / amax).view(-1, 1)
    else:
        scale = amax * (1.0 / top.double()).float()
        t = y32 / scale.view(-1, 1)
    return _e4m3_bytes(t, mut), scale


def _silu(g):
    return g / (1.0 + torch.exp(-g))


def _gelu(g):
    c = 0.7978845608028654
    return 0.5 * g * (1.0 + torch.tanh(c * (g + 0.044715 * g * g * g)))


def emulate(kernel, inp, mut=None):
    """fp32 emulation of `kernel` (optionally a mutant) -> outputs by name,
    as row_oracle.verify reads them."""
    out = {}
    if kernel in ro.GATED:
        g, u = inp["x"].float().chunk(2, dim=-1)
        if mut == "gate_up_swapped":
            g, u = u, g
        act = _gelu if kernel == "gelu_and_mul" else _silu
        if mut == "silu_for_gelu":
            act = _silu
        y32 = act(g) * u
        if kernel == "silu_and_mul_fp8":
            out["q"], out["scale"] = _quant(y32, "mul", mut)
        else:
            out["y"] = _bf16(y32, mut)
        return out
    if kernel in ("quant_fp8", "quant_fp8_div"):
        form = "div" if kernel == "quant_fp8_div" else "mul"
        out["q"], out["scale"] = _quant(inp["x"].float(), form, mut)
        return out

    w, eps = inp["w"].float(), inp["eps"]
    if kernel == "embed_rmsnorm_fp8":
        ids, V = inp["ids"].long(), inp["table"].shape[0]
        if mut == "embed_id_unclamped":
            idx = ids % V
        elif mut == "embed_row_from_previous_id":
            idx = ids.roll(1).clamp(0, V - 1)
        else:
            idx = ids.clamp(0, V - 1)
        out["x_out"] = inp["table"][idx]
        v = out["x_out"].float()
    elif kernel in ro.FUSED:
        v = inp["x"].float() + inp["r"].float()
        out["residual"] = v.bfloat16()
        if mut == "residual_rounded_before_norm":
            v = out["residual"].float()
    else:
        v = inp["x"].float()
    H = v.shape[-1]
    sq = v * v
    if mut == "sum_drops_needle_vector":
        vec = v.abs().argmax(-1) // 8
        cols = torch.arange(H).view(1, -1) // 8
        sq = torch.where(cols == vec.view(-1, 1), torch.zeros_like(sq), sq)
    n = H
    if mut == "mean_over_padded_length":
        threads, iters = ro.dispatch(H // 8, "norm")
        n = threads * iters * 8
    mean = sq.sum(-1, keepdim=True) / n
    if mut == "eps_omitted":
        inv = torch.rsqrt(mean)
    elif mut == "eps_outside_sqrt":
        inv = 1.0 / (torch.sqrt(mean) + eps)
    else:
        inv = torch.rsqrt(mean + eps)

    if kernel in ("rmsnorm", "fused_add_rmsnorm"):
        out["y"] = _bf16(v * inv * w, mut)
    elif kernel == "fused_add_rmsnorm_fp8_div":
        y32 = v * inv * w
        out["y"] = _bf16(y32, mut)
        src = y32 if mut == "div_row_not_rounded" else out["y"].float()
        out["q"], out["scale"] = _quant(src, "div", mut)
    else:
        y32 = v * (inv * w)
        before = v * inv if mut == "amax_before_weight" else None
        out["q"], out["scale"] = _quant(y32, "mul", mut, amax_of=before)
    return out


# ---------------------------------------------------------------------------
# accepted
# ---------------------------------------------------------------------------

_inputs = {}


def _inp(kernel, family, T, H):
    """Built once, shared, never modified."""
    key = (kernel, family, T, H)
    if key not in _inputs:
        _inputs[key] = ro.make_inputs(kernel, family, T, H)
    return _inputs[key]


@pytest.mark.parametrize("H", ro.WIDTHS)
@pytest.mark.parametrize("kernel", ro.KERNELS)
def test_accepts_fp32_emulation(kernel, H):
    for family in ro.families(kernel):
        for T in (1, 3):
            if family == "needle" and T == 1:
                continue  # the needle batch has its own row count
            inp = _inp(kernel, family, T, H)
            results = ro.verify(kernel, inp, emulate(kernel, inp))
            for r in results:
                print(f"ROW_EMU {kernel} H={H} {family} T={T} {r}")
            assert not ro.failures(results), (kernel, H, family, T)


def test_needle_rows_cover_every_iteration_boundary():
    assert ro.needle_vectors(8, "norm") == [0]
    assert ro.needle_vectors(2056, "norm") == [0, 255, 256]
    assert ro.needle_vectors(8200, "norm") == [
        0, 255, 256, 511, 512, 767, 768, 1023, 1024]
    assert ro.needle_vectors(8200, "max") == [0, 511, 512, 1023, 1024]
    assert ro.needle_vectors(16392, "norm")[-3:] == [1536, 2047, 2048]
    assert len(ro.needle_vectors(32768, "max")) == 16
    for kernel in ("rmsnorm_fp8", "quant_fp8"):
        x = ro.make_inputs(kernel, "needle", 1, 4104)["x"].double()
        assert x.shape[0] == 2 * len(ro.needle_vectors(4104, "norm"))
        energy = x.pow(2)
        assert bool((energy.amax(1) > 0.99 * energy.sum(1)).all())


def test_exact_share_is_a_condition():
    """Bytes that take the odd neighbour at an exact midpoint stay inside the
    hard bound, so only the cap can see them: 1 % of a call fails it, 0.4 %
    does not."""
    n = 4000
    t = torch.linspace(16.3, 31.7, n, dtype=torch.float64).view(1, n)
    scale = torch.ones(1)
    for ties, rejected in ((40, True), (16, False)):
        y = t.clone()
        y[0, :ties] = 17.0  # midway between the codes 16 and 18
        q = ro.rne_e4m3(y).float().to(ro.FP8).view(torch.uint8)
        q[0, :ties] = torch.tensor(18.0).to(ro.FP8).view(torch.uint8)
        res = ro.check_fp8(q, y, scale)
        assert res.worst <= 1.0  # the hard bound holds either way
        assert (not res.ok) == rejected, str(res)
        assert res.note.endswith("under 0.995") == rejected
        assert ro.check_fp8(q, y, scale, share=False).ok


@pytest.mark.parametrize("kernel", ("rmsnorm_fp8", "fused_add_rmsnorm_fp8",
                                    "embed_rmsnorm_fp8", "silu_and_mul_fp8"))
def test_zero_row_scale_is_pinned_to_the_bit(kernel):
    """Where check_scale is the scale's only check, one ulp on the all-zero
    row's scale (far inside EPS) is still rejected: that row is exact."""
    inp = _inp(kernel, "zeros", 3, 264)
    out = emulate(kernel, inp)
    assert not ro.failures(ro.verify(kernel, inp, out))
    want = ro.CLAMP_F32 / torch.tensor(ro.FP8_MAX)
    zero = (out["q"] == 0).all(-1)
    assert int(zero.sum()) == 1
    assert torch.equal(out["scale"][zero], want.view(1))
    off = dict(out, scale=torch.where(
        zero, torch.nextafter(want, torch.tensor(1.0)), out["scale"]))
    fails = ro.failures(ro.verify(kernel, inp, off))
    assert len(fails) == 1 and fails[0].startswith("zero-row scale bits")


# ---------------------------------------------------------------------------
# rejected
# ---------------------------------------------------------------------------

_FP8_OUT = tuple(k for k in ro.KERNELS if k.endswith("fp8") or "fp8_" in k)
_every = lambda H: True                                   # noqa: E731


def _padded(H):
    threads, iters = ro.dispatch(H // 8, "norm")
    return threads * iters * 8 != H


# mutant -> (widths it changes anything at, [(kernel, family that must
# reject it)])
MUTANTS = {
    "sum_drops_needle_vector": (_every, [
        ("rmsnorm", "needle"), ("fused_add_rmsnorm", "needle"),
        ("rmsnorm_fp8", "needle"), ("fused_add_rmsnorm_fp8_div", "needle"),
        ("embed_rmsnorm_fp8", "needle")]),
    "mean_over_padded_length": (_padded, [
        ("rmsnorm", "randn"), ("fused_add_rmsnorm_fp8", "randn")]),
    "eps_omitted": (_every, [
        ("rmsnorm", "tiny"), ("rmsnorm_fp8", "tiny"),
        ("fused_add_rmsnorm", "zeros")]),
    "eps_outside_sqrt": (_every, [
        ("rmsnorm", "tiny"), ("fused_add_rmsnorm_fp8", "tiny")]),
    "amax_misses_last_vector": (_every, [
        ("rmsnorm_fp8", "ramp"), ("rmsnorm_fp8", "needle"),
        ("fused_add_rmsnorm_fp8_div", "ramp"), ("quant_fp8", "ramp"),
        ("quant_fp8_div", "needle"), ("silu_and_mul_fp8", "ramp")]),
    "amax_before_weight": (_every, [
        ("rmsnorm_fp8", "randn"), ("embed_rmsnorm_fp8", "randn")]),
    "scale_amax_over_240": (_every, [(k, "randn") for k in _FP8_OUT]),
    "clamp_missing": (_every, [
        ("rmsnorm_fp8", "zeros"), ("fused_add_rmsnorm_fp8_div", "zeros"),
        ("quant_fp8", "tiny"), ("quant_fp8_div", "tiny"),
        ("quant_fp8", "zeros"), ("silu_and_mul_fp8", "tiny")]),
    "bf16_truncated": (_every, [
        ("rmsnorm", "randn"), ("fused_add_rmsnorm", "randn"),
        ("silu_and_mul", "randn"), ("gelu_and_mul", "randn")]),
    "fp8_truncated": (_every, [(k, "randn") for k in _FP8_OUT]),
    "residual_rounded_before_norm": (_every, [
        ("fused_add_rmsnorm", "randn")]),
    "div_row_not_rounded": (_every, [
        ("fused_add_rmsnorm_fp8_div", "randn")]),
    "gate_up_swapped": (_every, [(k, "randn") for k in ro.GATED]),
    "silu_for_gelu": (_every, [("gelu_and_mul", "randn")]),
    "embed_id_unclamped": (_every, [("embed_rmsnorm_fp8", "randn")]),
    "embed_row_from_previous_id": (_every, [("embed_rmsnorm_fp8", "randn")]),
}


@pytest.mark.parametrize(
    "mutant,H", [(m, H) for m in MUTANTS for H in ro.WIDTHS if MUTANTS[m][0](H)])
def test_rejects_mutant(mutant, H):
    for kernel, family in MUTANTS[mutant][1]:
        inp = _inp(kernel, family, 3, H)
        results = ro.verify(kernel, inp, emulate(kernel, inp, mutant))
        fails = ro.failures(results)
        print(f"ROW_MUTANT {mutant} {kernel} H={H} {family}: {fails}")
        assert fails, (mutant, kernel, H, family)
        if mutant == "sum_drops_needle_vector":
            # every needle position is seen: each row fails, not only some
            n_rows = (inp["ids"] if "ids" in inp else inp["x"]).shape[0]
            bad_rows = set().union(*(r.rows for r in results))
            assert bad_rows == set(range(n_rows)), (kernel, H, bad_rows)


def test_mean_over_padded_length_changes_nothing_at_full_rows():
    """Why that mutant is not asked for at 16384 and 32768: there the padded
    length IS the row length."""
    assert [H for H in ro.WIDTHS if not _padded(H)] == [16384, 32768]


@pytest.mark.parametrize("H", (264, 4104))
def test_structured_mutants_are_order_one(H):
    """The needle, tiny and ramp rows were built so that these defects are no
    marginal miss: at least 10x the bound."""
    for mutant, kernel, family in (
            ("sum_drops_needle_vector", "rmsnorm", "needle"),
            ("eps_omitted", "rmsnorm", "tiny"),
            ("eps_outside_sqrt", "rmsnorm", "tiny"),
            ("amax_misses_last_vector", "rmsnorm_fp8", "ramp")):
        inp = _inp(kernel, family, 3, H)
        results = ro.verify(kernel, inp, emulate(kernel, inp, mutant))
        assert max(r.worst for r in results) > 10, (mutant, H)
