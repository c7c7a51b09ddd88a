"""int4 (W4A16) decode GEMMs on the GPU: the fused dequant-GEMM kernel against
int4_dequant + F.linear and against ops.linear on the dequantized bf16 weight
(what the same AWQ checkpoint costs without quantization="int4").

    python scripts/bench_int4.py [--out table.md] [--capacity]
    python scripts/bench_int4.py --moe [--out table.md]

--moe times one Mixtral-8x7B MoE block with int4 experts (E = 8, k = 2,
H = 4096, I = 14336): the grouped path (ops.int4_moe_mlp) against the dense
expert loop of the same module (ops.INT4_MOE_T = 0), same method, the ring
being whole blocks; then int4_moe_gemm alone at 1, 2 and 4 column tiles per
workgroup, the sweep int4_moe_tiles' thresholds are read from.

Method: every call streams a DIFFERENT weight. Each route cycles through a
ring of weights of the same shape whose total size exceeds 512 MB, so no call
finds its weight in L2 or the 256 MB infinity cache. The calls of one ring
pass are captured in a graph (decode runs from graphs, and a single call is
shorter than its Python launch), replayed warm, then timed with device events
over several replays; the three routes alternate inside each repeat and the
median of the repeats is reported with its spread. Bytes are computed from
the shapes: the weight stream of the route, plus x and y.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import kubeai_amd.ops as ops  # noqa: E402
from kubeai_amd.engine.quant_int4 import Int4Weight  # noqa: E402

HBM_PEAK = 6.3e12  # bytes/s, the ceiling docs/kernels.md uses
SHAPES = [
    ("8B qkv", 6144, 4096), ("8B o", 4096, 4096),
    ("8B gate_up", 28672, 4096), ("8B down", 4096, 14336),
    ("70B qkv", 10240, 8192), ("70B o", 8192, 8192),
    ("70B gate_up", 57344, 8192), ("70B down", 8192, 28672),
]
MS = [1, 8, 16, 32, 48, 64, 128]  # 48: the one M-tile count the rest skips
RING_BYTES = 512 << 20
GROUP = 128


def random_int4(N, K, dev):
    """A packed weight with random codes: timing does not read the values."""
    G, kc = K // GROUP, (K + 127) // 128
    qp = torch.randint(-2**31, 2**31 - 1, (N // 16, kc, 64, 4),
                       dtype=torch.int32, device=dev)
    sp = (torch.rand(N // 16, G, 16, device=dev) * 0.01 + 0.001).half()
    zp = torch.randint(0, 256, (N // 16, G, 8), dtype=torch.uint8, device=dev)
    return Int4Weight(qp, sp, zp, N, K, GROUP)


def ring_of(make, nbytes):
    return [make() for _ in range(max(2, -(-RING_BYTES // nbytes)))]


class Route:
    """One ring pass of fn(x, w) captured in a graph."""

    def __init__(self, fn, x, ring):
        self.n = len(ring)
        for w in ring:  # warm every weight outside capture
            fn(x, w)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            for w in ring:
                self.y = fn(x, w)
        for _ in range(2):
            self.graph.replay()
        torch.cuda.synchronize()

    def time_us(self, min_calls=60):
        reps = max(2, -(-min_calls // self.n))
        s, e = torch.cuda.Event(True), torch.cuda.Event(True)
        s.record()
        for _ in range(reps):
            self.graph.replay()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / (reps * self.n)


def fused(x, w):
    ops.INT4_M_FUSED = 64
    return ops.int4_linear(x, w)


def dequant_linear(x, w):
    ops.INT4_M_FUSED = 0
    try:
        return ops.int4_linear(x, w)
    finally:
        ops.INT4_M_FUSED = 64


def bench(out_path):
    dev = "cuda"
    lines = [
        "| shape | N | K | M | fused us | dequant+linear us | bf16 linear us |"
        " fused vs dequant+linear | fused vs bf16 | fused GB/s | % of 6.3 TB/s |",
        "|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    ok_for_m = {m: True for m in MS if m <= 64}
    for name, N, K in SHAPES:
        w4_ring = ring_of(lambda: random_int4(N, K, dev), N * K // 2)
        bf_ring = ring_of(
            lambda: torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.02,
            N * K * 2,
        )
        w4_bytes = w4_ring[0].nbytes
        for M in MS:
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            routes = {}
            if M <= 64:
                routes["fused"] = Route(fused, x, w4_ring)
            routes["deq"] = Route(dequant_linear, x, w4_ring)
            routes["bf16"] = Route(ops.linear, x, bf_ring)
            samples = {k: [] for k in routes}
            for _ in range(5):
                for k, r in routes.items():
                    samples[k].append(r.time_us())
            med = {k: statistics.median(v) for k, v in samples.items()}
            spread = {
                k: (max(v) - min(v)) / med[k] * 100 for k, v in samples.items()
            }
            xy_bytes = M * K * 2 + M * N * 2
            if "fused" in med:
                f = med["fused"]
                bps = (w4_bytes + xy_bytes) / (f * 1e-6)
                ok_for_m[M] &= f <= med["deq"]
                cells = (f"{f:.1f} (±{spread['fused']:.0f}%)",
                         f"{med['deq'] / f:.2f}x", f"{med['bf16'] / f:.2f}x",
                         f"{bps / 1e9:.0f}", f"{bps / HBM_PEAK * 100:.0f}")
            else:
                cells = ("-", "-", "-", "-", "-")
            line = (
                f"| {name} | {N} | {K} | {M} | {cells[0]} | "
                f"{med['deq']:.1f} (±{spread['deq']:.0f}%) | "
                f"{med['bf16']:.1f} (±{spread['bf16']:.0f}%) | "
                f"{cells[1]} | {cells[2]} | {cells[3]} | {cells[4]} |"
            )
            print(line, flush=True)
            lines.append(line)
            del routes
        del w4_ring, bf_ring
        torch.cuda.empty_cache()
    verdict = "fused <= dequant+linear on every shape: " + ", ".join(
        f"M={m}: {'yes' if v else 'no'}" for m, v in ok_for_m.items()
    )
    print(verdict)
    lines += ["", verdict]
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def capacity():
    """Weight bytes resident after load, llama-3-8b, int4 against none."""
    from kubeai_amd.engine import EngineConfig, LLMEngine

    for quant in (None, "int4"):
        torch.cuda.empty_cache()
        torch.cuda.synchronize()
        eng = LLMEngine(EngineConfig(
            model="llama-3-8b", device="cuda", num_gpu_blocks=64,
            max_model_len=512, quantization=quant, enable_graphs=False,
        ))
        model = eng.runner.model
        nbytes = sum(
            t.numel() * t.element_size()
            for t in list(model.parameters()) + list(model.buffers())
        )
        print(f"capacity llama-3-8b quantization={quant}: model tensors "
              f"{nbytes / 1e9:.3f} GB, allocated "
              f"{torch.cuda.memory_allocated() / 1e9:.3f} GB", flush=True)
        del eng, model


# ------------------------------------------------------------------- --moe
MOE_E, MOE_K, MOE_H, MOE_I = 8, 2, 4096, 14336
MOE_TS = [1, 2, 4, 8, 16, 32, 64]


def random_moe_block(dev):
    """A MoEMLP of 8x7B dimensions whose experts are Int4Linears over random
    packed weights (no float weights are ever materialised)."""
    import dataclasses

    from kubeai_amd.engine.quant_int4 import Int4Linear
    from kubeai_amd.models.config import PRESETS
    from kubeai_amd.models.llama import MoEMLP

    cfg = dataclasses.replace(
        PRESETS["mixtral-tiny"], hidden_size=MOE_H, intermediate_size=MOE_I,
        num_local_experts=MOE_E, num_experts_per_tok=MOE_K,
    )
    with torch.device("meta"):
        mlp = MoEMLP(cfg)
    mlp.gate = torch.nn.Linear(MOE_H, MOE_E, bias=False, device=dev,
                               dtype=torch.bfloat16)
    for ex in mlp.experts:
        ex.gate_up_proj = Int4Linear(random_int4(2 * MOE_I, MOE_H, dev))
        ex.down_proj = Int4Linear(random_int4(MOE_H, MOE_I, dev))
    assert mlp.refresh_int4_groups() is not None
    return mlp


def moe_grouped(x, mlp):
    ops.INT4_MOE_T = 64
    return mlp(x)


def moe_dense(x, mlp):
    ops.INT4_MOE_T = 0
    try:
        return mlp(x)
    finally:
        ops.INT4_MOE_T = 64


def active_experts(x, ring):
    n = []
    for mlp in ring:
        router = torch.nn.functional.linear(x.float(), mlp.gate.weight.float())
        n.append(torch.topk(router, MOE_K, dim=-1).indices.unique().numel())
    return sum(n) / len(n)


def measure(routes, repeats=5, min_calls=40):
    samples = {k: [] for k in routes}
    for _ in range(repeats):
        for k, r in routes.items():
            samples[k].append(r.time_us(min_calls))
    med = {k: statistics.median(v) for k, v in samples.items()}
    spread = {k: (max(v) - min(v)) / med[k] * 100 for k, v in samples.items()}
    return med, spread


def bench_moe(out_path):
    from kubeai_amd import _C

    dev = "cuda"
    ring = [random_moe_block(dev) for _ in range(2)]
    expert_bytes = sum(
        lin.int4.nbytes for lin in (ring[0].experts[0].gate_up_proj,
                                    ring[0].experts[0].down_proj)
    )
    print(f"one block's experts: {MOE_E * expert_bytes / 1e6:.0f} MB packed, "
          f"ring of {len(ring)}", flush=True)
    # launches of the expert part, by construction of the two code paths:
    # 2 grouped GEMMs + silu_and_mul + combine, against zeros + scatter and,
    # per expert, 2 GEMMs + silu_and_mul + multiply + add (the first add is
    # an assignment)
    launches = (4, 2 + 5 * MOE_E - 1)
    lines = [
        "| T | active experts | grouped us | dense loop us | dense / grouped |"
        " grouped GB/s | % of 6.3 TB/s | dense GB/s | launches grouped / dense |",
        "|---|---|---|---|---|---|---|---|---|",
    ]
    best_t, still_ok = 0, True
    for T in MOE_TS:
        x = torch.randn(T, MOE_H, device=dev, dtype=torch.bfloat16)
        # both routes on the same inputs give the same output
        same = all(
            torch.equal(moe_grouped(x, mlp), moe_dense(x, mlp)) for mlp in ring
        )
        assert same, f"grouped != dense loop at T = {T}"
        act = active_experts(x, ring)
        routes = {"grouped": Route(moe_grouped, x, ring),
                  "dense": Route(moe_dense, x, ring)}
        med, spread = measure(routes)
        g, d = med["grouped"], med["dense"]
        noise = max(spread["grouped"], spread["dense"]) / 100
        still_ok = still_ok and g <= d * (1 + noise)
        if still_ok:
            best_t = T
        g_bps = act * expert_bytes / (g * 1e-6)
        d_bps = MOE_E * expert_bytes / (d * 1e-6)
        line = (
            f"| {T} | {act:.1f} | {g:.1f} (±{spread['grouped']:.0f}%) | "
            f"{d:.1f} (±{spread['dense']:.0f}%) | {d / g:.2f}x | "
            f"{g_bps / 1e9:.0f} | {g_bps / HBM_PEAK * 100:.0f} | "
            f"{d_bps / 1e9:.0f} | {launches[0]} / {launches[1]} |"
        )
        print(line, flush=True)
        lines.append(line)
        del routes
    verdict = (f"largest T with grouped <= dense loop at every measured T up "
               f"to it: {best_t}")
    print(verdict, flush=True)
    lines += ["", verdict, ""]

    # column tiles per workgroup of int4_moe_gemm alone
    lines += [
        "| projection | N | K | T | plan NT | NT=1 us | NT=2 us | NT=4 us |",
        "|---|---|---|---|---|---|---|---|",
    ]
    for name, N, K, row_div, attr in (
        ("gate_up", 2 * MOE_I, MOE_H, MOE_K, 0), ("down", MOE_H, MOE_I, 1, 1),
    ):
        groups = [mlp.int4_groups()[attr] for mlp in ring]
        for T in MOE_TS:
            x = torch.randn(T * MOE_K // row_div, K, device=dev,
                            dtype=torch.bfloat16)
            selected = torch.topk(
                torch.randn(T, MOE_E, device=dev), MOE_K, dim=-1
            ).indices
            y = torch.empty(T * MOE_K, N, device=dev, dtype=torch.bfloat16)
            mt, plan_nt = _C.int4_moe_plan(N, T, MOE_E, MOE_K)

            def gemm(nt):
                def fn(x_, grp):
                    _C.int4_moe_gemm(y, x_, selected, grp.table, row_div,
                                     MOE_E, N, K, GROUP, nt)
                    return y
                return fn

            routes = {nt: Route(gemm(nt), x, groups)
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
    ap.add_argument("--out", default=None, help="write the markdown table here")
    ap.add_argument("--capacity", action="store_true")
    ap.add_argument("--moe", action="store_true",
                    help="the 8x7B MoE block: grouped experts vs the dense loop")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_int4 needs a GPU"
    torch.manual_seed(0)
    if args.capacity:
        capacity()
    elif args.moe:
        bench_moe(args.out)
    else:
        bench(args.out)
