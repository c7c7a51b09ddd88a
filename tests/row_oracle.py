"""fp64 oracles, derived error bounds and input families for the row kernels
(csrc/row_kernels.hip, csrc/activation.hip): test_row_kernels_gpu.py on the
GPU, test_row_oracle.py for the CPU self-check of this checker. Plain torch
on the CPU; the extension is never touched here.

The oracles
-----------
All work in fp64 over the very bf16 tensors the kernel receives (bf16 widens
to fp64 exactly):

* rmsnorm:      ``y = v * (mean(v^2) + eps)^-1/2 * w``;
* fused add:    ``v = x + r`` UNROUNDED, and ``residual' = bf16(v)``. The sum
  of two bf16 values is either exact in fp32 or (exponents more than 16
  apart) rounds in fp32 to a value whose bits below the bf16 midpoint come
  from the small addend alone, never exactly a bf16 tie: rounding it to fp32
  and then to bf16, as the kernel does, equals rounding it once. So
  ``residual'`` is an exact condition;
* ``_div``:     the quantized row is ``bf16(y)``, the row fused_add_rmsnorm
  writes. That row is checked against ``y`` like any bf16 output, and the
  quantization is then checked as quant_fp8_div OF THE KERNEL'S OWN ROW,
  where the maximum is exact;
* gated:        ``silu(g) * u`` and tanh-``gelu(g) * u`` over [gate | up];
* embed:        row ``clamp(ids[t], 0, V - 1)`` of the table.

The bounds
----------
``EPS = 2**-16`` is the relative error allowed to an fp32 evaluation of any
of these expressions; it is derived, not read off a kernel:

* norm. A thread sums at most 64 squares, then 6 wave steps and at most 16
  wave partials: fewer than 100 fp32 roundings (2**-24 each) on a sum of
  non-negative terms, under 2**-17.4 relative, halved by the square root.
  ``total / H + eps`` and ``rsqrtf`` add a few ulp, the two products two
  more, the fp32 ``x + r`` one. Under 2**-17 in all; EPS is that, doubled.
  The extension is built without -ffast-math (setup.py), so ``/`` is the
  IEEE division.
* silu. ``x / (1 + __expf(-x))``: ``__expf`` is the hardware exp2 after one
  fp32 product with log2(e), so the relative error of the exponential is
  about ``|x| * 2**-23``. The families keep ``|gate| <= 16``: under 2**-19,
  and the sum, the division and the product with ``up`` add 3 roundings.
  EPS holds.
* gelu. ``0.5 * x * (1 + tanhf(u))``, ``u = c * (x + 0.044715 x^3)``. ``u``
  carries about 4 roundings, which move tanh by ``(1 - t^2) |u| 2**-22 <=
  0.45 * 2**-22``. No ocml accuracy table is installed with the toolchain
  this was written against, so tanhf is taken at the OpenCL conformance
  limit, 5 ulp: ``<= 5 * 2**-23`` absolute, as ``|t| <= 1``. With the
  rounding of ``1 + t`` the factor ``1 + t`` is off by less than ``14 *
  2**-24 < 2**-20`` ABSOLUTE. For negative gates ``1 + t`` cancels, so that
  error is not relative to the result: the bound gets the absolute term
  ``GELU_ABS * |g * u|`` with ``GELU_ABS = 0.5 * 2**-20 = 8 * 2**-24``, next
  to EPS for the remaining products.

bf16 output:  ``|out - y| <= ulp_bf16(y) / 2 + EPS * |y| + TINY`` (round to
nearest of a value within EPS of y). ``TINY = 2**-126``, the smallest normal
fp32, below which a product may be flushed.

Row scale:    ``|scale - max(amax(y), 1e-6) / 448| <= EPS * that``. Where the
quantized row is bf16 (quant_fp8, quant_fp8_div, the ``_div`` norm) the
maximum is exact and the scale must have the fp32 BITS of ``amax / 448``
(multiplication form, common.h::row_scale_fp8) or ``amax * fp32(1 / 448)``
(division form, row_scale_fp8_div).

fp8 bytes, given the kernel's own scale ``s`` (checked above): with ``t = y /
s`` in fp64, saturated at +-448, the decoded byte must satisfy ``|dec - t| <=
step_e4m3(t) / 2 + EPS * |t|``, where the e4m3 step is ``2**(floor(log2 |t|)
- 3)``, at least the subnormal step 2**-9. And at least ``EXACT_SHARE = 99.5
%`` of a call's bytes must EQUAL round-to-nearest-even of ``t``: a chain with
relative error EPS misses the rounding only where ``t`` lies within EPS of a
midpoint, a share of about ``2 EPS / 2**-4`` = 0.05 %; the cap is ten times
that. A row whose oracle is all zero must be all zero bytes, and its scale
must have the bits of ``fp32(1e-6) / 448`` in the form's arithmetic.

The cap presumes that ``t`` is spread over the step. Where the quantized row
is bf16 (quant_fp8, quant_fp8_div, the ``_div`` norm) it is not: a bf16 value
times a power of two has 8 significant bits, so whenever ``448 / amax`` is a
power of two a sixteenth of a row sits EXACTLY on a midpoint, and ``y / s``
with the rounded ``s`` falls to either side of it (found with the fp32
emulation: 4 of 264 bytes of a randn row with amax 3.5). For those kernels
the cap is replaced by the stronger condition that is available there: every
byte equals ``exact_bytes``, the form's own chain of single IEEE fp32
operations evaluated by torch. The hard bound against fp64 stays.

The norm kernels feel the same effect, diluted: there ``t = 448 * (v_j w_j) /
(v_m w_m)`` is a ratio of products of two bf16 values, which lands exactly on
a midpoint whenever the odd part of the row maximum's product is small, and
most often in the ``cancel`` family, whose ``v`` keeps two or three
significant bits. The share of bytes that differ from the rounding of the
fp64 target is therefore not the 0.05 % of the estimate above but up to 0.41
% for the fp32 emulation (cancel, T = 1, H = 32768) and 0.28 % for the
kernels (cancel, H = 4104); every such byte sits on a tie and within the hard
bound. The 99.5 % cap is kept as it is. Its margin over those figures
belongs to the fixed seeds of the families: how many ties a row holds depends
on the draw, so a changed seed or family can move a call's share by tenths of
a percent without any defect, and a call that then falls under the cap has to
be looked at byte by byte (are the misses on ties?) before it is read as one.

Non-finite inputs are out of scope: every family is finite and any
non-finite output fails every check.

Input families
--------------
``rows(family, T, H, seed)`` returns bf16 [T, H]:

* ``randn``  — the generic case.
* ``needle`` — noise ``2**-6 * randn`` plus one element of magnitude 64 per
  row, one row per needle position (T is ignored): vectors 0 and nvec - 1 and,
  for every iteration boundary of the dispatched block width, ``it * threads
  - 1`` and ``it * threads``; elements 0 and 7 of the vector. The needle has
  over 99 % of the row's energy and is its maximum: a vector lost from the
  sum or from the amax is a 10x error in every output of the row. Norm
  weights are ``1 + 0.1 * randn`` so it stays the maximum after weighting.
  silu_and_mul and gelu_and_mul (activation.hip) are grid-stride kernels with
  no such iteration boundaries; they get the norm policy's rows only so that
  every kernel sees every family, and are elementwise anyway.
* ``tiny``   — ``2**-10 * randn``: mean square ~1e-6, below eps = 1e-5, so a
  missing or misplaced eps is an O(1) error. For the max-only kernels every
  second row has amax exactly 2**-24, under the 1e-6 clamp.
* ``zeros``  — an all-zero row among randn rows.
* ``large``  — ``randn * 2**k``, k uniform in 0..28 per element, clipped at
  2**30: squares (and a row's sum of them, < 2**78) stay finite in fp32.
* ``ramp``   — ``|x[i]| = (i + 1) / H`` with random signs and the last vector
  times 4: the largest element sits in the ragged tail without dominating
  the sum.
* ``cancel`` — fused kernels only: ``residual = -x + 2**-6 * randn``.

For the fused kernels x and residual are separate draws (for ``needle`` and
``ramp`` the residual is ``2**-6 * randn`` noise, so the structure survives
the sum). Gated inputs keep ``|gate| <= 16``.

Shapes
------
``WIDTHS`` are the smallest row lengths that reach every branch of
row_kernels.hip::dispatch_row with a ragged last iteration, the exact 256 x 8
boundary and the family's limit; ``dispatch`` mirrors dispatch_row.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import torch

EPS = 2.0 ** -16
GELU_ABS = 2.0 ** -21
TINY = 2.0 ** -126
EXACT_SHARE = 0.995
NORM_EPS = 1e-5

FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
# the clamp and the reciprocal as the kernels hold them, in fp32
CLAMP_F32 = torch.tensor(1e-6, dtype=torch.float32)
RCP448_F32 = torch.tensor(1.0 / 448.0, dtype=torch.float32)

WIDTHS = (8, 264, 2056, 4104, 8200, 16384, 16392, 32768)

NORM_KERNELS = ("rmsnorm", "fused_add_rmsnorm", "rmsnorm_fp8",
                "fused_add_rmsnorm_fp8", "fused_add_rmsnorm_fp8_div",
                "embed_rmsnorm_fp8")
MAX_KERNELS = ("silu_and_mul_fp8", "quant_fp8", "quant_fp8_div")
ACT_KERNELS = ("silu_and_mul", "gelu_and_mul")
KERNELS = NORM_KERNELS + MAX_KERNELS + ACT_KERNELS
FUSED = ("fused_add_rmsnorm", "fused_add_rmsnorm_fp8",
         "fused_add_rmsnorm_fp8_div")
GATED = ("silu_and_mul_fp8", "silu_and_mul", "gelu_and_mul")

_BASE = ("randn", "needle", "tiny", "zeros", "large", "ramp")


def families(kernel):
    return _BASE + (("cancel",) if kernel in FUSED else ())


def policy(kernel):
    return "max" if kernel in MAX_KERNELS else "norm"


def dispatch(nvec, pol):
    """(threads, iterations) row_kernels.hip::dispatch_row picks."""
    if nvec <= 256:
        return 256, 1
    if nvec <= 512:
        return 256, 2
    if nvec <= 1024:
        return 256, 4
    if pol == "norm":
        return (256, 8) if nvec <= 2048 else (512, 8)
    return (512, 4) if nvec <= 2048 else (512, 8)


def needle_vectors(H, pol):
    nvec = H // 8
    threads, iters = dispatch(nvec, pol)
    vecs = {0, nvec - 1}
    for it in range(1, iters):
        vecs |= {v for v in (it * threads - 1, it * threads) if v < nvec}
    return sorted(vecs)


def needle_positions(H, pol):
    return [v * 8 + e for v in needle_vectors(H, pol) for e in (0, 7)]


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (hash(k) if isinstance(k, int) else
                                  sum(map(ord, k)))) % (2 ** 31)
    return torch.Generator().manual_seed(seed)


def _rows_f32(family, T, H, gen, pol="norm"):
    def randn(*s):
        return torch.randn(*s, generator=gen)

    if family == "randn":
        return randn(T, H)
    if family == "needle":
        pos = needle_positions(H, pol)
        x = 2.0 ** -6 * randn(len(pos), H)
        for p, at in enumerate(pos):
            x[p, at] = 64.0 if p % 2 == 0 else -64.0
        return x
    if family == "tiny":
        x = 2.0 ** -10 * randn(T, H)
        if pol == "max":
            for t in range(1, T, 2):
                r = randn(H)
                x[t] = r / r.abs().amax() * 2.0 ** -24
        return x
    if family == "zeros":
        x = randn(T, H)
        x[T // 2] = 0.0
        return x
    if family == "large":
        k = torch.randint(0, 29, (T, H), generator=gen)
        return (randn(T, H) * torch.exp2(k.float())).clamp(-2.0 ** 30, 2.0 ** 30)
    if family == "ramp":
        sign = torch.randint(0, 2, (T, H), generator=gen).float() * 2 - 1
        x = sign * (torch.arange(1, H + 1).float() / H)
        x[:, -8:] *= 4.0
        return x
    raise ValueError(family)


def rows(family, T, H, seed=0, pol="norm"):
    return _rows_f32(family, T, H, _gen(family, T, H, seed), pol).bfloat16()


def norm_weight(H, seed=0):
    return (1.0 + 0.1 * torch.randn(H, generator=_gen("w", H, seed))).bfloat16()


def pair(family, T, H, seed=0):
    """(x, residual) of a fused kernel."""
    gen = _gen("pair", family, T, H, seed)
    if family == "cancel":
        x = torch.randn(T, H, generator=gen).bfloat16()
        r = -x.float() + 2.0 ** -6 * torch.randn(T, H, generator=gen)
        return x, r.bfloat16()
    x = _rows_f32(family, T, H, gen)
    if family in ("needle", "ramp"):
        r = 2.0 ** -6 * torch.randn(x.shape, generator=gen)
    else:
        r = _rows_f32(family, T, H, gen)
        if family == "zeros":
            r[T // 2] = 0.0
    return x.bfloat16(), r.bfloat16()


def gated(family, T, I, seed=0, pol="norm"):
    """[T, 2I] packed [gate | up], |gate| <= 16, whose product silu(g) * u
    has the family's structure."""
    gen = _gen("gated", family, T, I, seed)
    up = _rows_f32(family, T, I, gen, pol)
    gate = (2.0 * torch.randn(up.shape, generator=gen)).clamp(-16.0, 16.0)
    if family == "needle":
        gate *= 2.0 ** -4
        for p, at in enumerate(needle_positions(I, pol)):
            gate[p, at] = 16.0
            up[p, at] = 4.0 if p % 2 == 0 else -4.0
    elif family == "tiny":
        up *= 2.0 ** -20  # products under the 1e-6 clamp
    elif family == "zeros":
        gate[up.shape[0] // 2] = 0.0  # silu(0) * 0 = +0, not -0
    elif family == "ramp":
        gate = torch.full_like(up, 2.0)
    return torch.cat([gate, up], dim=1).bfloat16()


def make_inputs(kernel, family, T, H, seed=0):
    """The CPU inputs of one call, by argument name. For ``needle`` the
    batch is one row per needle position and T is ignored."""
    pol = policy(kernel)
    if kernel in GATED:
        return dict(x=gated(family, T, H, seed, pol))
    if kernel in MAX_KERNELS:
        return dict(x=rows(family, T, H, seed, pol))
    inp = dict(w=norm_weight(H, seed), eps=NORM_EPS)
    if kernel in FUSED:
        inp["x"], inp["r"] = pair(family, T, H, seed)
    elif kernel == "embed_rmsnorm_fp8":
        table = rows(family, 5, H, seed)  # needle: one row per position
        V = table.shape[0]
        if family == "needle":
            # every table row, out of order, with ids beyond both ends
            ids = ([V + 3, -1] + list(range(V - 1, -1, -1))
                   + [-(2 ** 31), 2 ** 31 - 1])
        else:
            ids = [-1, V + 3, 2][:T]  # rows 0, V - 1 and (zeros) the zero row
        inp["table"] = table
        inp["ids"] = torch.tensor(ids, dtype=torch.int32)
    else:
        inp["x"] = rows(family, T, H, seed)
    return inp


def row_slice(kernel, inp, t):
    """The inputs of the one-row call on row t of `inp`."""
    one = dict(inp)
    for k in ("x", "r", "ids"):
        if k in inp:
            one[k] = inp[k][t:t + 1].clone()
    return one


# ---------------------------------------------------------------------------
# oracles
# ---------------------------------------------------------------------------

def f64(t):
    return t.float().double()  # bf16 widens exactly


def oracle_rmsnorm(v, w, eps):
    return v * (v.pow(2).mean(-1, keepdim=True) + eps).rsqrt() * f64(w)


def oracle_embed_rows(table, ids):
    return table[ids.long().clamp(0, table.shape[0] - 1)]


def oracle_silu_mul(x):
    g, u = f64(x).chunk(2, dim=-1)
    return g / (1.0 + torch.exp(-g)) * u


def oracle_gelu_mul(x):
    g, u = f64(x).chunk(2, dim=-1)
    c = 0.7978845608028654  # sqrt(2 / pi)
    return 0.5 * g * (1.0 + torch.tanh(c * (g + 0.044715 * g ** 3))) * u


def round_bf16(v64):
    """bf16 of an fp64 tensor that holds sums of two bf16 values (exact, see
    the module docstring)."""
    return v64.float().bfloat16()


# ---------------------------------------------------------------------------
# checkers
# ---------------------------------------------------------------------------

@dataclass
class Result:
    what: str
    bad: int            # elements over the bound
    n: int
    worst: float        # max err / bound (inf for a non-finite output)
    at: tuple = ()      # index of the worst element
    rows: list = field(default_factory=list)  # rows with a bad element
    note: str = ""

    @property
    def ok(self):
        return self.bad == 0

    def __str__(self):
        return (f"{self.what}: {self.bad} of {self.n} over the bound, worst "
                f"err/bound {self.worst:.3g} at {self.at}, rows "
                f"{self.rows[:16]} {self.note}")


def _floor_log2(a):
    return torch.frexp(a)[1] - 1


def ulp_bf16(y):
    e = _floor_log2(y.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(y), e - 7)


def step_e4m3(t):
    e = _floor_log2(t.abs().clamp(2.0 ** -6, FP8_MAX))
    return torch.ldexp(torch.ones_like(t), e - 3)


def rne_e4m3(t):
    tc = t.clamp(-FP8_MAX, FP8_MAX)
    st = step_e4m3(tc)
    return (torch.round(tc / st) * st).clamp(-FP8_MAX, FP8_MAX)  # half to even


def _result(what, err, bound, extra_bad=None, note=""):
    ratio = err / bound
    ratio = torch.where(torch.isfinite(ratio), ratio,
                        torch.full_like(ratio, float("inf")))
    bad = ratio > 1.0
    if extra_bad is not None:
        bad = bad | extra_bad
    flat = int(ratio.argmax())
    at = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat),
                                                   ratio.shape))
    rows_ = bad.reshape(bad.shape[0], -1).any(1).nonzero().flatten().tolist()
    return Result(what, int(bad.sum()), bad.numel(), float(ratio.max()), at,
                  rows_, note)


def check_bf16(out, y, what="bf16", abs_term=None):
    assert out.dtype == torch.bfloat16 and out.shape == y.shape, (
        out.dtype, out.shape, y.shape)
    bound = ulp_bf16(y) / 2 + EPS * y.abs() + TINY
    if abs_term is not None:
        bound = bound + abs_term
    return _result(what, (out.double() - y).abs(), bound)


def check_equal(got, want, what):
    """Bit equality of two tensors of one dtype."""
    assert got.dtype == want.dtype and got.shape == want.shape, (
        what, got.dtype, want.dtype, got.shape, want.shape)
    bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[got.element_size()]
    ne = (got.contiguous().view(bits) != want.contiguous().view(bits))
    ne = ne.reshape(ne.shape[0], -1) if ne.dim() else ne.reshape(1, 1)
    err = ne.double()
    return _result(what, err, torch.full_like(err, 0.5))


def want_scale(y):
    """fp64 max(amax(y), 1e-6) / 448 per row."""
    return y.abs().amax(-1).clamp_min(float(CLAMP_F32)) / FP8_MAX


def check_scale(scale, y, what="scale"):
    assert scale.dtype == torch.float32 and scale.shape == y.shape[:1]
    want = want_scale(y)
    return _result(what, (scale.double() - want).abs().view(-1, 1),
                   (EPS * want).view(-1, 1))


def exact_scale(xb, form):
    """fp32 scale of a bf16 row batch, whose maximum is exact."""
    amax = torch.maximum(xb.float().abs().amax(-1), CLAMP_F32)
    return amax / torch.tensor(FP8_MAX) if form == "mul" else amax * RCP448_F32


def check_scale_exact(scale, xb, form, what="scale bits"):
    assert scale.dtype == torch.float32 and scale.shape == xb.shape[:1]
    return check_equal(scale.view(-1, 1), exact_scale(xb, form).view(-1, 1),
                       what)


def check_zero_row_scale(scale, y, what="zero-row scale bits"):
    """An all-zero oracle row comes from exact zeros (v = 0, or silu(0) * 0 =
    +0), so the kernel's amax is exactly 0 and its scale must have the bits
    of fmaxf(0, 1e-6f) / 448.0f, the multiplication form: within EPS is not
    enough there."""
    zero = (y == 0).all(-1)
    want = torch.where(zero, exact_scale(torch.zeros(1, 8).bfloat16(), "mul"),
                       scale)
    return check_equal(scale.view(-1, 1), want.view(-1, 1), what)


def exact_bytes(xb, form):
    """The e4m3 bytes of a bf16 row batch in the fp32 arithmetic of `form`
    (common.h::quant8_fp8 / quant8_fp8_div): every step is one IEEE fp32
    operation, so torch reproduces it bit for bit."""
    amax = torch.maximum(xb.float().abs().amax(-1, keepdim=True), CLAMP_F32)
    if form == "mul":
        t = xb.float() * (torch.tensor(FP8_MAX) / amax)
    else:
        t = xb.float() / (amax * RCP448_F32)
    return t.clamp(-FP8_MAX, FP8_MAX).to(FP8).view(torch.uint8)


def check_fp8(q, y, scale, what="fp8", share=True):
    """q: uint8 [T, W] e4m3 bytes; y: fp64 oracle row; scale: the kernel's
    own fp32 row scales. share=False leaves the exact-share cap out (bf16
    rows, which get check_equal against exact_bytes instead)."""
    assert q.dtype == torch.uint8 and q.shape == y.shape, (q.dtype, q.shape)
    dec = q.view(FP8).float().double()
    s = scale.double().view(-1, 1)
    s = torch.where((s > 0) & torch.isfinite(s), s,
                    torch.full_like(s, float("nan")))
    t = (y / s).clamp(-FP8_MAX, FP8_MAX)
    bound = step_e4m3(t) / 2 + EPS * t.abs()
    zero_rows = (y == 0).all(-1, keepdim=True)
    res = _result(what, (dec - t).abs(), bound, extra_bad=zero_rows & (q != 0))
    exact = dec == rne_e4m3(t)
    exact_share = float(exact.double().mean())
    res.note = f"exact share {exact_share:.5f}"
    if share and exact_share < EXACT_SHARE:
        miss = ~exact
        res.bad = max(res.bad, int(miss.sum()))
        res.rows = sorted(set(res.rows) |
                          set(miss.any(1).nonzero().flatten().tolist()))
        res.note += f" under {EXACT_SHARE}"
    return res


# ---------------------------------------------------------------------------
# one call: outputs against the oracle
# ---------------------------------------------------------------------------

def verify(kernel, inp, out):
    """All checks of one call. `inp` as make_inputs returns it; `out` by
    name, as the implementation under test returned it on the CPU:
      y         bf16 output (for the in-place kernels, x afterwards)
      residual  residual afterwards (fused)
      q, scale  e4m3 bytes as uint8, fp32 row scales (fp8 out)
      x_out     gathered rows (embed)
    Returns the list of Results."""
    res = []
    if kernel in ACT_KERNELS:
        g, u = f64(inp["x"]).chunk(2, dim=-1)
        if kernel == "silu_and_mul":
            res.append(check_bf16(out["y"], oracle_silu_mul(inp["x"])))
        else:
            res.append(check_bf16(out["y"], oracle_gelu_mul(inp["x"]),
                                  abs_term=GELU_ABS * (g * u).abs()))
        return res
    if kernel in ("quant_fp8", "quant_fp8_div"):
        form = "div" if kernel == "quant_fp8_div" else "mul"
        res.append(check_scale_exact(out["scale"], inp["x"], form))
        res.append(check_fp8(out["q"], f64(inp["x"]), out["scale"],
                             share=False))
        res.append(check_equal(out["q"], exact_bytes(inp["x"], form),
                               "fp8 bytes"))
        return res
    if kernel == "silu_and_mul_fp8":
        y = oracle_silu_mul(inp["x"])
        res.append(check_scale(out["scale"], y))
        res.append(check_zero_row_scale(out["scale"], y))
        res.append(check_fp8(out["q"], y, out["scale"]))
        return res

    # norm kernels
    if kernel == "embed_rmsnorm_fp8":
        xrows = oracle_embed_rows(inp["table"], inp["ids"])
        res.append(check_equal(out["x_out"], xrows, "x_out"))
        v = f64(xrows)
    elif kernel in FUSED:
        v = f64(inp["x"]) + f64(inp["r"])
        res.append(check_equal(out["residual"], round_bf16(v), "residual'"))
    else:
        v = f64(inp["x"])
    y = oracle_rmsnorm(v, inp["w"], inp["eps"])
    if kernel in ("rmsnorm", "fused_add_rmsnorm"):
        res.append(check_bf16(out["y"], y))
    elif kernel == "fused_add_rmsnorm_fp8_div":
        res.append(check_bf16(out["y"], y, "bf16 row"))
        res.append(check_scale_exact(out["scale"], out["y"], "div"))
        res.append(check_fp8(out["q"], f64(out["y"]), out["scale"],
                             share=False))
        res.append(check_equal(out["q"], exact_bytes(out["y"], "div"),
                               "fp8 bytes"))
    else:
        res.append(check_scale(out["scale"], y))
        res.append(check_zero_row_scale(out["scale"], y))
        res.append(check_fp8(out["q"], y, out["scale"]))
    return res


def failures(results):
    return [str(r) for r in results if not r.ok]
