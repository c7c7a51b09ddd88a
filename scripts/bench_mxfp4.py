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


TILED_MS = [65, 128, 256, 512, 1024, 2048, 8192]
TILED_FORMS = [(64, 128), (64, 64)]


def bench_tiled(out_path, ms, names):
    """mxfp4_gemm_tiled for M > 64 against the route it replaces
    (mxfp4_dequant + F.linear), with bf16 ops.linear and fp8 _scaled_mm for
    context, every tile form forced beside the planned one. Same method as
    bench(): cold weights from a ring, all routes alternating, median of 5."""
    from kubeai_amd.engine.quant import Fp8Linear

    dev = "cuda"
    forms = [f"{bm}x{bn}" for bm, bn in TILED_FORMS]
    lines = [
        "| shape | N | K | M | plan | tiled us | quant_fp8 + tiled us |"
        " dequant+linear us | bf16 linear us | fp8 _scaled_mm us | tiled TF |"
        " tiled GB/s | " + " | ".join(f"{f} us" for f in forms) + " |",
        "|" + "---|" * (12 + len(forms)),
    ]
    ok_for_m = {m: True for m in ms}
    for name, N, K in SHAPES:
        if names and name not in names:
            continue
        mx_ring = ring_of(lambda: random_mxfp4(N, K, dev), N * K // 2)
        bf_ring = ring_of(
            lambda: torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02,
            N * K * 2,
        )
        f8_ring = ring_of(lambda: Fp8Linear(bf_ring[0]).to(dev), N * K)
        for M in ms:
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            xq, xs = ops.quant_fp8(x)
            y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)

            def tiled(form):
                def fn(_, w):
                    _C.mxfp4_gemm_tiled(y, xq, xs, w.qp, w.sp, N, K, *form)
                    return y
                return fn

            def quant_tiled(x_, w):
                q8, s8 = ops.quant_fp8(x_)
                _C.mxfp4_gemm_tiled(y, q8, s8, w.qp, w.sp, N, K)
                return y

            def dequant_linear(x_, w):
                dense = ops.mxfp4_dequant(w, out=ops.dequant_workspace(w.device, N, K))
                return torch.nn.functional.linear(x_, dense)

            routes = {
                "tiled": Route(tiled((0, 0)), x, mx_ring),
                "module": Route(quant_tiled, x, mx_ring),
                "deq": Route(dequant_linear, x, mx_ring),
                "bf16": Route(ops.linear, x, bf_ring),
                "fp8": Route(lambda _, lin: lin.forward_quantized(xq, xs), x, f8_ring),
            }
            for f, form in zip(forms, TILED_FORMS):
                routes[f] = Route(tiled(form), x, mx_ring)
            # a ring pass at M = 8192 is tens of milliseconds: fewer calls
            med, spread = measure(routes, min_calls=max(4, min(60, 16384 // M)))
            ok_for_m[M] &= med["module"] <= med["deq"]
            t = med["tiled"] * 1e-6
            nbytes = mx_ring[0].nbytes + M * K + 4 * M + 2 * M * N
            bm, bn = _C.mxfp4_tiled_plan(M, N)
            cell = lambda k: f"{med[k]:.1f} (±{spread[k]:.0f}%)"
            line = (
                f"| {name} | {N} | {K} | {M} | {bm}x{bn} | {cell('tiled')} | "
                f"{cell('module')} | {cell('deq')} | {cell('bf16')} | {cell('fp8')} | "
                f"{2 * M * N * K / t / 1e12:.0f} | {nbytes / t / 1e9:.0f} | "
                + " | ".join(cell(f) for f in forms) + " |"
            )
            print(line, flush=True)
            lines.append(line)
            del routes
        del mx_ring, bf_ring, f8_ring
        torch.cuda.empty_cache()
    verdict = "quant_fp8 + tiled <= dequant+linear on every shape run: " + ", ".join(
        f"M={m}: {'yes' if v else 'no'}" for m, v in ok_for_m.items()
    )
    print(verdict)
    lines += ["", verdict]
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def engine_ab(repeats):
    """llama-3-8b with random weights under mxfp4, KUBEAI_MXFP4_TILED_M unset
    against set, alternating: 16 prompts of 100 - 2000 tokens, 32 new tokens
    each; tok/s over the whole run and the time to the first token of each
    request, with the spread of the repeats."""
    import random
    import statistics
    import time

    from kubeai_amd.engine import EngineConfig, LLMEngine, SamplingParams

    rng = random.Random(0)
    prompts = [
        [rng.randrange(10, 30000) for _ in range(rng.randrange(100, 2001))]
        for _ in range(16)
    ]
    eng = LLMEngine(EngineConfig(
        model="llama-3-8b", device="cuda", num_gpu_blocks=4096,
        max_model_len=4096, quantization="mxfp4", max_num_batched_tokens=2048,
        # the same prompts come back in every run: without this the measured
        # runs would admit them as prefix-cache hits and prefill nothing
        enable_prefix_caching=False,
    ))

    def run(tag):
        t0 = time.perf_counter()
        for i, p in enumerate(prompts):
            eng.add_request(p, SamplingParams(max_tokens=32, ignore_eos=True),
                            request_id=f"{tag}{i}")
        first, n_tok = {}, 0
        while eng.has_work():
            for o in eng.step():
                first.setdefault(o.request_id, time.perf_counter() - t0)
                if o.finished:
                    n_tok += len(o.output_token_ids)
        torch.cuda.synchronize()
        return n_tok / (time.perf_counter() - t0), statistics.mean(first.values())

    res = {"off": [], "on": []}
    for r in range(repeats + 1):  # the first pair warms up and is dropped
        for mode in ("off", "on"):
            os.environ.pop("KUBEAI_MXFP4_TILED_M", None)
            if mode == "on":
                os.environ["KUBEAI_MXFP4_TILED_M"] = "2048"
            out = run(f"{mode}{r}_")
            if r:
                res[mode].append(out)
    for mode, v in res.items():
        tps, ttft = [a for a, _ in v], [b for _, b in v]
        print(f"engine A/B switch {mode}: tok/s median {statistics.median(tps):.0f} "
              f"(min {min(tps):.0f}, max {max(tps):.0f}), mean TTFT median "
              f"{statistics.median(ttft) * 1e3:.0f} ms (min {min(ttft) * 1e3:.0f}, "
              f"max {max(ttft) * 1e3:.0f})", flush=True)


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
    ap.add_argument("--tiled", action="store_true",
                    help="sweep mxfp4_gemm_tiled at M > 64")
    ap.add_argument("--ms", type=int, nargs="*", default=TILED_MS)
    ap.add_argument("--shapes", nargs="*", default=None,
                    help='with --tiled: shape names, e.g. "8B qkv"')
    ap.add_argument("--engine-ab", type=int, default=0, metavar="REPEATS",
                    help="llama-3-8b, KUBEAI_MXFP4_TILED_M off against on")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mxfp4 needs a GPU"
    torch.manual_seed(0)
    if args.capacity:
        capacity()
    elif args.tiled:
        bench_tiled(args.out, args.ms, args.shapes)
    elif args.engine_ab:
        engine_ab(args.engine_ab)
    else:
        bench(args.out)
