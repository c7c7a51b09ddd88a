"""paged_attention_append on the GPU against the route it replaces
(_C.paged_attention_prefill: v1 at B = 1, the 4-wave v2 form at B > 1) on a few
new query rows per sequence over a long cached context, and the sweep of its
split target.

    python scripts/bench_append.py [--out table.md] [--quick]

Method of bench_int4.py / bench_mxfp4.py: every call reads a different set of
cache blocks from a ring larger than 512 MB (cold cache), one ring pass is
captured in a graph, timed with device events, routes alternating, median of 5
repeats. The split count of a target is append_n_splits' rule evaluated here,
so one process sweeps all targets.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_int4 import HBM_PEAK, Route, measure  # noqa: E402

import torch  # noqa: E402

from kubeai_amd import _C  # noqa: E402

HD, BS = 128, 16
TQS = [4, 16, 48]
BATCHES = [1, 4]
CTXS = [1024, 4096, 16384, 65536]
HEADS = [(32, 8), (64, 8)]
TARGETS = [256, 512, 1024, 2048]
RING_BYTES = 512 << 20


def n_splits_for(target, Tq, B, n_kv, max_blocks):
    """attn_plan::append_n_splits with `target` in place of its constant."""
    wgs = B * n_kv * (-(-Tq // 16))
    n = min(16, -(-target // wgs)) if wgs < target else 1
    return min(n, max(1, -(-max_blocks // 2)))


def bench(out_path, quick):
    dev = "cuda"
    n_kv = 8
    ctxs = CTXS[:2] if quick else CTXS
    per_seq = max(ctxs) // BS + 4               # blocks of the longest sequence
    pool_blocks = 2 * max(BATCHES) * per_seq + 1
    pools = {}
    k = torch.empty(pool_blocks, n_kv, BS, HD, device=dev, dtype=torch.bfloat16).normal_()
    v = torch.empty_like(k).normal_()
    pools["bf16"] = (k, v)
    pools["e5m2"] = (k.to(torch.float8_e5m2), v.to(torch.float8_e5m2))
    lines = [
        "| heads | cache | B | Tq/seq | ctx | parent plan | parent us | "
        + " | ".join(f"T={t} us (S)" for t in TARGETS)
        + " | best/parent | KV GB/s at best | % of 6.3 TB/s |",
        "|" + "---|" * (10 + len(TARGETS)),
    ]
    records = []
    for n_q, _ in HEADS:
        for cache, (kc, vc) in pools.items():
            for B in BATCHES:
                for tq in TQS:
                    for ctx in ctxs:
                        L = ctx + tq
                        nblk = -(-L // BS)
                        Tq = B * tq
                        entry_bytes = 2 * B * nblk * n_kv * BS * HD * kc.element_size()
                        n_ring = max(2, -(-RING_BYTES // entry_bytes))
                        n_ring = min(n_ring, (pool_blocks - 1) // (B * nblk))
                        ring = []
                        for i in range(n_ring):
                            ids = torch.randperm(B * nblk) + 1 + i * B * nblk
                            ring.append(ids.view(B, nblk).to(torch.int32).to(dev))
                        q = torch.randn(Tq, n_q, HD, device=dev).to(torch.bfloat16)
                        out = torch.empty_like(q)
                        qsl = torch.arange(0, Tq + 1, tq, dtype=torch.int32, device=dev)
                        sl = torch.full((B,), L, dtype=torch.int32, device=dev)
                        scale = HD ** -0.5

                        def parent(_, bt):
                            _C.paged_attention_prefill(out, q, kc, vc, bt, qsl, sl, scale, 0, 0.0)
                            return out

                        def append(S):
                            def fn(_, bt):
                                _C.paged_attention_append(out, q, kc, vc, bt, qsl, sl, scale, S)
                                return out
                            return fn

                        splits = {t: n_splits_for(t, Tq, B, n_kv, nblk) for t in TARGETS}
                        routes = {"parent": Route(parent, None, ring)}
                        for S in sorted(set(splits.values())):
                            routes[S] = Route(append(S), None, ring)
                        med, spread = measure(routes, min_calls=8 if ctx >= 16384 else 40)
                        best = min(med[S] for S in set(splits.values()))
                        kv_bytes = entry_bytes
                        plan = _C.prefill_plan(Tq, B, n_q, n_kv, HD, nblk)
                        cells = " | ".join(
                            f"{med[splits[t]]:.1f} ({splits[t]})" for t in TARGETS)
                        line = (
                            f"| {n_q}/{n_kv} | {cache} | {B} | {tq} | {ctx} | v{plan[0]} x{plan[1]} | "
                            f"{med['parent']:.1f} (±{spread['parent']:.0f}%) | {cells} | "
                            f"{best / med['parent']:.2f} | {kv_bytes / best / 1e3:.0f} | "
                            f"{kv_bytes / (best * 1e-6) / HBM_PEAK * 100:.0f} |"
                        )
                        print(line, flush=True)
                        lines.append(line)
                        records.append(dict(
                            n_q=n_q, cache=cache, B=B, tq=tq, ctx=ctx,
                            parent=med["parent"],
                            append={t: med[splits[t]] for t in TARGETS},
                            splits=splits))
                        del routes, ring
    # per target and context: append <= parent at every swept (Tq, B, heads, cache)
    lines.append("")
    for t in TARGETS:
        row = []
        for ctx in ctxs:
            rs = [r for r in records if r["ctx"] == ctx]
            worst = max(r["append"][t] / r["parent"] for r in rs)
            row.append(f"ctx {ctx}: worst append/parent {worst:.2f}")
        total = sum(r["append"][t] / r["parent"] for r in records) / len(records)
        lines.append(f"target {t}: " + "; ".join(row) + f"; mean ratio {total:.3f}")
        print(lines[-1], flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        with open(os.path.splitext(out_path)[0] + ".json", "w") as fh:
            json.dump(records, fh)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the markdown table here")
    ap.add_argument("--quick", action="store_true", help="contexts 1k and 4k only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_append needs a GPU"
    torch.manual_seed(0)
    bench(args.out, args.quick)
