"""One Mixtral-8x7B MoE block with fp8 experts (E = 8, k = 2, H = 4096,
I = 14336) on the GPU: the grouped path (ops.fp8_moe_mlp, KUBEAI_FP8_MOE_T=64)
against the dense expert loop of the same module (the switch at 0, which is
the default), then fp8_moe_gemm alone at 1, 2 and 4 column tiles per
workgroup, the sweep fp8_moe_tiles' floor is read from.

    python scripts/bench_fp8_moe.py [--out table.md]

Method, as in bench_int4.py --moe (profiles/r10_int4_moe.md): every call
streams a DIFFERENT block. The routes cycle through a ring of blocks, each
1.4 GB of expert weights, so no call finds its weights in L2 or the 256 MB
infinity cache. One ring pass is captured in a graph, replayed warm, then
timed with device events over several replays; the routes alternate inside
each of 5 repeats and the median is reported with (max - min) / median.
The two routes do not give the same bits (another summation order); their
distance is what tests/test_fp8_moe_gpu.py bounds.
"""
import argparse
import dataclasses
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

from bench_int4 import HBM_PEAK, Route, active_experts, measure  # noqa: E402
from kubeai_amd.engine.quant import FP8_DTYPE, Fp8Linear  # noqa: E402
from kubeai_amd.models.config import PRESETS  # noqa: E402
from kubeai_amd.models.llama import MoEMLP  # noqa: E402

MOE_E, MOE_K, MOE_H, MOE_I = 8, 2, 4096, 14336
MOE_TS = [1, 2, 4, 8, 16, 32, 64]
RING = 2
SWITCH = "KUBEAI_FP8_MOE_T"


def random_fp8_linear(N, K, dev):
    """An Fp8Linear over random finite e4m3 bytes (no float weight is ever
    materialised): timing does not read the values."""
    lin = Fp8Linear(torch.zeros(16, 32, dtype=torch.bfloat16))
    mag = torch.randint(0, 0x78, (N, K), dtype=torch.uint8, device=dev)
    sign = torch.randint(0, 2, (N, K), dtype=torch.uint8, device=dev) << 7
    lin.weight_fp8 = (mag | sign).view(FP8_DTYPE)
    lin.weight_scale = torch.rand(1, N, device=dev) * 1e-4 + 1e-5
    lin.out_features, lin.in_features = N, K
    return lin


def random_moe_block(dev):
    cfg = dataclasses.replace(
        PRESETS["mixtral-tiny"], hidden_size=MOE_H, intermediate_size=MOE_I,
        num_local_experts=MOE_E, num_experts_per_tok=MOE_K,
    )
    with torch.device("meta"):
        mlp = MoEMLP(cfg)
    mlp.gate = torch.nn.Linear(MOE_H, MOE_E, bias=False, device=dev,
                               dtype=torch.bfloat16)
    for ex in mlp.experts:
        ex.gate_up_proj = random_fp8_linear(2 * MOE_I, MOE_H, dev)
        ex.down_proj = random_fp8_linear(MOE_H, MOE_I, dev)
    assert mlp.refresh_fp8_groups() is not None
    return mlp


def moe_grouped(x, mlp):
    os.environ[SWITCH] = "64"
    try:
        return mlp(x)
    finally:
        os.environ[SWITCH] = "0"


def moe_dense(x, mlp):
    os.environ[SWITCH] = "0"
    return mlp(x)


def bench(out_path):
    from kubeai_amd import _C

    dev = "cuda"
    ring = [random_moe_block(dev) for _ in range(RING)]
    expert_bytes = (2 * MOE_I * MOE_H + MOE_H * MOE_I) + 4 * (2 * MOE_I + MOE_H)
    print(f"one block's experts: {MOE_E * expert_bytes / 1e6:.0f} MB, "
          f"ring of {len(ring)}", flush=True)
    # launches of the expert part, by construction of the two code paths:
    # quant + 2 grouped GEMMs + silu_and_mul_fp8 + combine, against zeros +
    # scatter + quant and, per expert, 2 GEMMs + silu_and_mul_fp8 + multiply
    # + add (the first add is an assignment)
    launches = (5, 3 + 5 * MOE_E - 1)
    lines = [
        "| T | active experts | grouped us | dense loop us | dense / grouped |"
        " grouped GB/s | % of 6.3 TB/s | dense GB/s | rel. distance |"
        " launches grouped / dense |",
        "|---|---|---|---|---|---|---|---|---|---|",
    ]
    faster = []
    for T in MOE_TS:
        x = torch.randn(T, MOE_H, device=dev, dtype=torch.bfloat16)
        g0, d0 = moe_grouped(x, ring[0]).float(), moe_dense(x, ring[0]).float()
        dist = ((g0 - d0).norm() / d0.norm()).item()
        act = active_experts(x, ring)
        routes = {"grouped": Route(moe_grouped, x, ring),
                  "dense": Route(moe_dense, x, ring)}
        med, spread = measure(routes)
        g, d = med["grouped"], med["dense"]
        noise = max(spread["grouped"], spread["dense"]) / 100
        faster.append((T, g * (1 + noise) < d))
        g_bps = act * expert_bytes / (g * 1e-6)
        d_bps = MOE_E * expert_bytes / (d * 1e-6)
        line = (
            f"| {T} | {act:.1f} | {g:.1f} (±{spread['grouped']:.0f}%) | "
            f"{d:.1f} (±{spread['dense']:.0f}%) | {d / g:.2f}x | "
            f"{g_bps / 1e9:.0f} | {g_bps / HBM_PEAK * 100:.0f} | "
            f"{d_bps / 1e9:.0f} | {dist:.1e} | {launches[0]} / {launches[1]} |"
        )
        print(line, flush=True)
        lines.append(line)
        del routes
    verdict = "grouped faster than the dense loop beyond the spread: " + ", ".join(
        f"T={t}: {'yes' if ok else 'no'}" for t, ok in faster
    )
    print(verdict, flush=True)
    lines += ["", verdict, ""]

    # column tiles per workgroup of fp8_moe_gemm alone
    lines += [
        "| projection | N | K | T | plan NT | NT=1 us | NT=2 us | NT=4 us |",
        "|---|---|---|---|---|---|---|---|",
    ]
    for name, N, K, row_div, attr in (
        ("gate_up", 2 * MOE_I, MOE_H, MOE_K, 0), ("down", MOE_H, MOE_I, 1, 1),
    ):
        groups = [mlp.fp8_groups()[attr] for mlp in ring]
        for T in MOE_TS:
            R = T * MOE_K // row_div
            xq = torch.randn(R, K, device=dev).to(FP8_DTYPE)
            xs = torch.rand(R, device=dev) + 0.5
            selected = torch.topk(
                torch.randn(T, MOE_E, device=dev), MOE_K, dim=-1
            ).indices
            y = torch.empty(T * MOE_K, N, device=dev, dtype=torch.bfloat16)
            mt, plan_nt = _C.fp8_moe_plan(N, T, MOE_E, MOE_K)

            def gemm(nt):
                def fn(x_, grp):
                    _C.fp8_moe_gemm(y, x_, xs, selected, grp.table, row_div,
                                    MOE_E, N, K, nt)
                    return y
                return fn

            routes = {nt: Route(gemm(nt), xq, groups)
                      for nt in (1, 2, 4) if mt * nt < 16}
            med, spread = measure(routes)
            cells = [
                f"{med[nt]:.1f} (±{spread[nt]:.0f}%)" if nt in med else "-"
                for nt in (1, 2, 4)
            ]
            line = (f"| {name} | {N} | {K} | {T} | {plan_nt} | "
                    + " | ".join(cells) + " |")
            print(line, flush=True)
            lines.append(line)
            del routes
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the markdown tables here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fp8_moe needs a GPU"
    torch.manual_seed(0)
    bench(args.out)
