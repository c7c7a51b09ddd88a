"""Multi-LoRA decode timings on the GPU (profiles/r12_lora.md).

  apply : LoRAManager.apply's per-adapter sgmv loop (host clock, its syncs
          included) against ops.lora_apply (graph replay), 8B shapes
  sweep : ops.lora_apply over the K splits, the data behind _C.lora_plan
  step  : an 8B decode step of 40 rows, 4 adapters spread over the rows:
          eager with the sgmv loop (KUBEAI_LORA_BATCHED_T=0, the step before
          the batched path) against the captured graph; and without adapters

Every timed call rotates over COPIES sets of adapter weights, as the layers of
a model do, so A and B are not served from one warm line set. One JSON line
per measurement on stdout.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kubeai_amd import ops  # noqa: E402
from kubeai_amd.engine.lora import LoRAManager, LoraTable  # noqa: E402

SHAPES = {  # target -> (K, N) of llama-3-8b
    "qkv": (4096, 6144), "o": (4096, 4096),
    "gate_up": (4096, 28672), "down": (14336, 4096),
}
COPIES = 8


def emit(**kw):
    print(json.dumps(kw), flush=True)


def graph_us(fn, replays: int) -> float:
    """Microseconds per replay of fn captured once (device events)."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(3):
        g.replay()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(replays):
        g.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / replays


def host_us(fn, iters: int) -> float:
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


def make_case(K, N, R, T, n_adapters):
    """COPIES tables with n_adapters rank-R adapters each; rows dealt out to
    the adapters in turn, every fifth row base."""
    g = torch.Generator().manual_seed(K + N + R + T)
    tables, adapters = [], []
    for _ in range(COPIES):
        table, by_id = LoraTable(K, N, "cuda"), {}
        for a in range(1, n_adapters + 1):
            A = (torch.randn(R, K, generator=g) * 0.05).bfloat16().cuda()
            B = (torch.randn(N, R, generator=g) * 0.5).bfloat16().cuda()
            table.set_row(a, A, B, 2.0 / R)
            by_id[a] = {"t": [(A, B, 2.0 / R)]}
        tables.append(table)
        adapters.append(by_id)
    ids = [0 if t % 5 == 4 else 1 + t % n_adapters for t in range(T)]
    ids = torch.tensor(ids, dtype=torch.int32, device="cuda")
    x = torch.randn(T, K, generator=g).bfloat16().cuda()
    y = torch.zeros(T, N, dtype=torch.bfloat16, device="cuda")
    return tables, adapters, ids, x, y


def run_apply(args):
    vpart = ops.lora_vpart("cuda")
    for tgt, (K, N) in SHAPES.items():
        for R in (16, 64):
            for T in (1, 8, 32, 64):
                for n in (1, 4):
                    tables, adapters, ids, x, y = make_case(K, N, R, T, n)

                    def old():
                        for by_id in adapters:
                            LoRAManager.apply(
                                SimpleNamespace(adapters=by_id), 0, "t", x, y, ids
                            )

                    def new(ks=0):
                        for table in tables:
                            ops.lora_apply(y, x, ids, table, vpart, ks)

                    emit(kind="apply", target=tgt, K=K, N=N, R=R, T=T, adapters=n,
                         sgmv_loop_us=host_us(old, args.iters) / COPIES,
                         batched_eager_us=host_us(new, args.iters) / COPIES,
                         batched_graph_us=graph_us(new, args.iters) / COPIES)


def run_sweep(args):
    vpart = ops.lora_vpart("cuda")
    for tgt in ("qkv", "down"):
        K, N = SHAPES[tgt]
        for R in (16, 64):
            for T in (8, 64):
                for n in (1, 4):
                    tables, _, ids, x, y = make_case(K, N, R, T, n)
                    us = {}
                    for ks in (1, 2, 4, 8, 16, 32):
                        def new():
                            for table in tables:
                                ops.lora_apply(y, x, ids, table, vpart, ks)
                        us[ks] = round(graph_us(new, args.iters) / COPIES, 2)
                    emit(kind="sweep", target=tgt, K=K, R=R, T=T, adapters=n,
                         plan=ops._C.lora_plan(T, K)[1], us_by_ks=us)


def run_step(args):
    from kubeai_amd.engine import EngineConfig, LLMEngine, SamplingParams
    from kubeai_amd.engine.scheduler import Request, ScheduledSeq, SchedulerOutput

    eng = LLMEngine(EngineConfig(model="llama-3-8b", device="cuda",
                                 max_model_len=2048, num_gpu_blocks=1024, seed=0))
    runner, ctx, rows = eng.runner, 128, 40

    def step(n_adapters):
        seqs = []
        for i in range(rows):
            lid = 0 if n_adapters == 0 or i % 5 == 4 else 1 + i % n_adapters
            req = Request(list(range(100, 101 + ctx)), SamplingParams(max_tokens=4),
                          request_id=f"r{i}", lora_id=lid)
            req.block_table = list(range(1 + 9 * i, 10 + 9 * i))
            seqs.append(ScheduledSeq(req, ctx, 1))
        return SchedulerOutput(decode=seqs, prefill=[], preempted=[])

    def ms(so):
        return host_us(lambda: runner.execute(so, 0), args.steps) / 1e3

    emit(kind="step", adapters=0, path="graph", ms=ms(step(0)))
    for a in range(1, 5):
        runner.load_lora(a, None)
    os.environ["KUBEAI_LORA_BATCHED_T"] = "0"
    emit(kind="step", adapters=4, path="eager + sgmv loop", ms=ms(step(4)))
    del os.environ["KUBEAI_LORA_BATCHED_T"]
    emit(kind="step", adapters=4, path="graph + batched", ms=ms(step(4)))
    emit(kind="step", adapters=4, path="graph + batched, all rows base",
         ms=ms(step(0)))
    for a in range(1, 5):
        runner.unload_lora(a)
    emit(kind="step", adapters=0, path="graph, after unload", ms=ms(step(0)))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("what", choices=["apply", "sweep", "step"])
    p.add_argument("--iters", type=int, default=40)
    p.add_argument("--steps", type=int, default=30)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lora.py measures on the GPU; none found")
    with torch.inference_mode():
        {"apply": run_apply, "sweep": run_sweep, "step": run_step}[args.what](args)


if __name__ == "__main__":
    main()
