"""The packed-row prefill kernel (G = 5, 6, 7) on the GPU against v2 on the
neighbouring group sizes G = 4 and 8: fresh causal prefill of one sequence.

    python scripts/bench_packed.py [--out table.md] [--quick]

Method of bench_append.py (bench_int4.py's Route and measure): every call
reads another set of randperm cache blocks from a ring, one ring pass is
captured in a graph, timed with device events, routes alternating, median of 5
repeats. TF counts the causal half only: 4 * 128 * n_q * Tq * (Tq + 1) / 2.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_int4 import Route, measure  # noqa: E402

import torch  # noqa: E402

from kubeai_amd import _C  # noqa: E402

HD, BS = 128, 16
TQS = [512, 2048, 8192]
N_KVS = [4, 8]
GS = [4, 5, 6, 7, 8]  # 4 and 8 run v2
RING_BYTES = 256 << 20


def bench(out_path, quick):
    dev = "cuda"
    tqs = TQS[:2] if quick else TQS
    lines = [
        "| n_kv | cache | Tq | " + " | ".join(
            f"{'v2' if G in (4, 8) else 'packed'} G={G} TF" for G in GS)
        + " | " + " | ".join(f"G={G} / slower v2" for G in (5, 6, 7)) + " |",
        "|" + "---|" * (3 + len(GS) + 3),
    ]
    for n_kv in N_KVS:
        nblk_max = max(tqs) // BS
        k = torch.empty(2 * nblk_max + 1, n_kv, BS, HD, device=dev,
                        dtype=torch.bfloat16).normal_()
        v = torch.empty_like(k).normal_()
        pools = {"bf16": (k, v),
                 "e5m2": (k.to(torch.float8_e5m2), v.to(torch.float8_e5m2))}
        for cache, (kc, vc) in pools.items():
            for Tq in tqs:
                nblk = Tq // BS
                entry = 2 * nblk * n_kv * BS * HD * kc.element_size()
                n_ring = min(max(2, RING_BYTES // entry), (k.shape[0] - 1) // nblk)
                ring = [(torch.randperm(nblk) + 1 + i * nblk).view(1, nblk)
                        .to(torch.int32).to(dev) for i in range(n_ring)]
                qsl = torch.tensor([0, Tq], dtype=torch.int32, device=dev)
                sl = torch.tensor([Tq], dtype=torch.int32, device=dev)
                scale = HD ** -0.5
                # a captured graph holds raw addresses and Route keeps only the
                # output: every input stays referenced here until the routes
                # are gone (torch.cuda.graph empties the allocator's cache on
                # entry, which would unmap a q that had been dropped)
                routes, flops, keep = {}, {}, [kc, vc, qsl, sl]
                for G in GS:
                    q = torch.randn(Tq, n_kv * G, HD, device=dev).to(torch.bfloat16)
                    out = torch.empty_like(q)
                    keep += [q, out]
                    flops[G] = 4 * HD * n_kv * G * Tq * (Tq + 1) / 2
                    if G in (4, 8):
                        assert _C.prefill_plan(Tq, 1, n_kv * G, n_kv, HD, nblk)[0] == 2
                    else:
                        assert _C.packed_prefill_plan(Tq, 1, n_kv * G, n_kv, HD, nblk)[0]

                    def prefill(_, bt, q=q, out=out):
                        _C.paged_attention_prefill(out, q, kc, vc, bt, qsl, sl, scale, 0, 0.0)
                        return out

                    routes[G] = Route(prefill, None, ring)
                med, spread = measure(routes, min_calls=8 if Tq >= 8192 else 40)
                tf = {G: flops[G] / (t * 1e-6) / 1e12 for G, t in med.items()}
                slower = min(tf[4], tf[8])
                line = (f"| {n_kv} | {cache} | {Tq} | "
                        + " | ".join(f"{tf[G]:.1f} (±{spread[G]:.0f}%)" for G in GS)
                        + " | " + " | ".join(f"{tf[G] / slower:.2f}" for G in (5, 6, 7))
                        + " |")
                print(line, flush=True)
                lines.append(line)
                del routes, ring, keep
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the markdown table here")
    ap.add_argument("--quick", action="store_true", help="Tq 512 and 2048 only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_packed needs a GPU"
    torch.manual_seed(0)
    bench(args.out, args.quick)
