"""MXFP4 (W4A8) decode GEMMs on the GPU: mxfp4_gemm against int4_gemm
(g = 128), bf16 ops.linear and the mxfp4_dequant + F.linear route, the module's
bf16-input route (quant_fp8 + mxfp4_gemm, two launches), then mxfp4_gemm alone
at 1, 2 and 4 column tiles per workgroup.

    python scripts/bench_mxfp4.py [--out table.md] [--capacity]

Method, shapes and helpers are bench_int4.py's: every call streams a
different weight from a ring larger than 512 MB, one ring pass is captured in
a graph, timed with device events, routes alternating, median of 5 repeats.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_int4 import (  # noqa: E402
    HBM_PEAK, SHAPES, Route, measure, random_int4, ring_of,
)

import torch  # noqa: E402

import kubeai_amd.ops as ops  # noqa: E402
from kubeai_amd import _C  # noqa: E402
from kubeai_amd.engine.quant_mxfp4 import Mxfp4Linear, Mxfp4Weight  # noqa: E402

MS = [1, 16, 32, 64]


def random_mxfp4(N, K, dev):
    """A packed weight with random codes and exponents 120..134: timing does
    not read the values."""
    kc = (K + 127) // 128
    J = ((kc + 7) // 8 + 3) // 4
    qp = torch.randint(0, 256, (N // 16, kc, 64, 16), dtype=torch.uint8, device=dev)
    sp = torch.randint(120, 135, (N // 16, J, 8, 64, 4), dtype=torch.uint8, device=dev)
    return Mxfp4Weight(qp, sp, N, K)


def bench(out_path):
    dev = "cuda"
    lines = [
        "| shape | N | K | M | plan MT x NT | mxfp4 us | int4 us | bf16 linear us |"
        " mxfp4 dequant+linear us | quant_fp8 + mxfp4 us | mxfp4 GB/s |"
        " % of 6.3 TB/s | NT=1 us | NT=2 us | NT=4 us |",
        "|" + "---|" * 15,
    ]
    ok_for_m = {m: True for m in MS}
    for name, N, K in SHAPES:
        mx_ring = ring_of(lambda: random_mxfp4(N, K, dev), N * K // 2)
        i4_ring = ring_of(lambda: random_int4(N, K, dev), N * K // 2)
        bf_ring = ring_of(
            lambda: torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02,
            N * K * 2,
        )
        lin_ring = [Mxfp4Linear(w) for w in mx_ring]
        big = torch.randn(65, K, device=dev, dtype=torch.bfloat16)
        for M in MS:
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            xq, xs = ops.quant_fp8(x)
            y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)

            def gemm(nt):
                def fn(_, w):
                    _C.mxfp4_gemm(y, xq, xs, w.qp, w.sp, N, K, nt)
                    return y
                return fn

            def dequant_linear(x_, w):
                dense = ops.mxfp4_dequant(w, out=ops.dequant_workspace(w.device, N, K))
                return torch.nn.functional.linear(x_, dense)

            routes = {
                "mxfp4": Route(lambda _, w: ops.mxfp4_linear(xq, xs, w), x, mx_ring),
                "int4": Route(ops.int4_linear, x, i4_ring),
                "bf16": Route(ops.linear, x, bf_ring),
                "deq": Route(dequant_linear, x, mx_ring),
                # Mxfp4Linear.forward on bf16 rows: what a caller outside the
                # fused layer branch (LoRA steps) pays
                "module": Route(lambda x_, lin: lin(x_), x, lin_ring),
            }
            for nt in (1, 2, 4):
                if (N // 16) % nt == 0:
                    routes[nt] = Route(gemm(nt), x, mx_ring)
            med, spread = measure(routes, min_calls=60)
            f = med["mxfp4"]
            ok_for_m[M] &= max(f, med["module"]) <= med["deq"]
            bps = (mx_ring[0].nbytes + M * K + 4 * M + 2 * M * N) / (f * 1e-6)
            mt, nt_plan = _C.mxfp4_plan(M, N)
            cell = lambda k: f"{med[k]:.1f} (±{spread[k]:.0f}%)" if k in med else "-"
            line = (
                f"| {name} | {N} | {K} | {M} | {mt} x {nt_plan} | {cell('mxfp4')} | "
                f"{cell('int4')} | {cell('bf16')} | {cell('deq')} | {cell('module')} | "
                f"{bps / 1e9:.0f} | "
                f"{bps / HBM_PEAK * 100:.0f} | {cell(1)} | {cell(2)} | {cell(4)} |"
            )
            print(line, flush=True)
            lines.append(line)
            del routes
        # the module's own M = 65 route runs (dequant + F.linear), untimed
        lin_ring[0](big)
        del mx_ring, lin_ring, i4_ring, bf_ring
        torch.cuda.empty_cache()
    verdict = "mxfp4, with and without quant_fp8, <= dequant+linear on every shape: " + ", ".join(
        f"M={m}: {'yes' if v else 'no'}" for m, v in ok_for_m.items()
    )
    print(verdict)
    lines += ["", verdict]
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def capacity():
    """Weight bytes resident after load, llama-3-8b under mxfp4."""
    from kubeai_amd.engine import EngineConfig, LLMEngine

    eng = LLMEngine(EngineConfig(
        model="llama-3-8b", device="cuda", num_gpu_blocks=64,
        max_model_len=512, quantization="mxfp4", enable_graphs=False,
    ))
    model = eng.runner.model
    nbytes = sum(
        t.numel() * t.element_size()
        for t in list(model.parameters()) + list(model.buffers())
    )
    print(f"capacity llama-3-8b quantization=mxfp4: model tensors "
          f"{nbytes / 1e9:.3f} GB, allocated "
          f"{torch.cuda.memory_allocated() / 1e9:.3f} GB", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the markdown table here")
    ap.add_argument("--capacity", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mxfp4 needs a GPU"
    torch.manual_seed(0)
    if args.capacity:
        capacity()
    else:
        bench(args.out)
