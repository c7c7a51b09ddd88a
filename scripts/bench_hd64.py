"""The head_dim 64 attention kernels on the GPU next to their hd-128
yardsticks.

    python scripts/bench_hd64.py [--out table.md] [--quick]

Decode: B x L = 2048 at 32/8 and 14/2 heads (Llama-3.2-1B, Qwen2.5-0.5B),
both caches, against the hd-128 kernel at EQUAL KV bytes (same B, L and G,
half the kv heads); GB/s counts the K and V bytes of the batch once.
Prefill: one fresh causal sequence, the same head shapes against the hd-128
route with equal n_kv (v2 at G = 4, packed at G = 7); TF counts the causal
half only, 4 * hd * n_q * Tq * (Tq + 1) / 2.

Method of bench_packed.py (bench_int4.py's Route and measure): every call
reads another set of randperm cache blocks from a ring, one ring pass is
captured in a graph, timed with device events, routes alternating, median of
5 repeats.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_int4 import Route, measure  # noqa: E402

import torch  # noqa: E402

from kubeai_amd import _C  # noqa: E402

BS = 16
SHAPES = [(32, 8), (14, 2)]  # (n_q, n_kv) at hd 64
DTYPES = {"bf16": torch.bfloat16, "e5m2": torch.float8_e5m2}


def _pool(n_blocks, n_kv, hd, dtype, dev):
    k = torch.empty(n_blocks + 1, n_kv, BS, hd, device=dev,
                    dtype=torch.bfloat16).normal_()
    return k.to(dtype), torch.empty_like(k).normal_().to(dtype)


def bench_decode(lines, quick, dev="cuda"):
    L, n_ring = 2048, 2
    nblk = L // BS
    lines += ["| heads | cache | B | hd 64 us | hd 64 GB/s | hd 128 us | "
              "hd 128 GB/s | hd 64 / hd 128 |", "|" + "---|" * 8]
    for n_q, n_kv in SHAPES:
        G = n_q // n_kv
        for cache, dtype in DTYPES.items():
            for B in ([64] if quick else [64, 256]):
                routes, keep = {}, []
                sl = torch.full((B,), L, dtype=torch.int32, device=dev)
                ring = [(torch.randperm(B * nblk) + 1 + i * B * nblk)
                        .view(B, nblk).to(torch.int32).to(dev)
                        for i in range(n_ring)]
                for hd, nkv in ((64, n_kv), (128, n_kv // 2)):
                    kc, vc = _pool(n_ring * B * nblk, nkv, hd, dtype, dev)
                    q = torch.randn(B, nkv * G, hd, device=dev).to(torch.bfloat16)
                    out = torch.empty_like(q)
                    keep += [kc, vc, q, out]

                    def decode(_, bt, q=q, out=out, kc=kc, vc=vc, hd=hd):
                        _C.paged_attention_decode(out, q, kc, vc, bt, sl,
                                                  hd ** -0.5, 0, 0.0)
                        return out

                    routes[hd] = Route(decode, None, ring)
                med, spread = measure(routes, min_calls=40)
                nbytes = 2 * B * L * n_kv * 64 * torch.empty(0, dtype=dtype).element_size()
                gbs = {hd: nbytes / (t * 1e-6) / 1e9 for hd, t in med.items()}
                line = (f"| {n_q}/{n_kv} | {cache} | {B} | "
                        f"{med[64]:.1f} (±{spread[64]:.0f}%) | {gbs[64]:.0f} | "
                        f"{med[128]:.1f} (±{spread[128]:.0f}%) | {gbs[128]:.0f} | "
                        f"{gbs[64] / gbs[128]:.2f} |")
                print(line, flush=True)
                lines.append(line)
                del routes, ring, keep


def bench_prefill(lines, quick, dev="cuda"):
    tqs = [512, 2048] if quick else [512, 2048, 8192]
    lines += ["", "| heads | cache | Tq | hd 64 TF | hd 128 TF (route) | "
              "hd 64 / hd 128 |", "|" + "---|" * 6]
    for n_q, n_kv in SHAPES:
        for cache, dtype in DTYPES.items():
            pools = {hd: _pool(4 * max(tqs) // BS, n_kv, hd, dtype, dev)
                     for hd in (64, 128)}
            for Tq in tqs:
                nblk = Tq // BS
                ring = [(torch.randperm(nblk) + 1 + i * nblk).view(1, nblk)
                        .to(torch.int32).to(dev) for i in range(4)]
                qsl = torch.tensor([0, Tq], dtype=torch.int32, device=dev)
                sl = torch.tensor([Tq], dtype=torch.int32, device=dev)
                routes, keep, tf = {}, [qsl, sl], {}
                for hd in (64, 128):
                    kc, vc = pools[hd]
                    q = torch.randn(Tq, n_q, hd, device=dev).to(torch.bfloat16)
                    out = torch.empty_like(q)
                    keep += [q, out]

                    def prefill(_, bt, q=q, out=out, kc=kc, vc=vc, hd=hd):
                        _C.paged_attention_prefill(out, q, kc, vc, bt, qsl, sl,
                                                   hd ** -0.5, 0, 0.0)
                        return out

                    routes[hd] = Route(prefill, None, ring)
                assert _C.hd64_prefill_plan(Tq, 1, n_q, n_kv, 64, nblk)[0]
                route = ("packed" if _C.packed_prefill_plan(
                    Tq, 1, n_q, n_kv, 128, nblk)[0] else
                    "v%d/%d waves" % _C.prefill_plan(Tq, 1, n_q, n_kv, 128, nblk))
                med, spread = measure(routes, min_calls=8 if Tq >= 8192 else 40)
                for hd, t in med.items():
                    tf[hd] = 4 * hd * n_q * Tq * (Tq + 1) / 2 / (t * 1e-6) / 1e12
                line = (f"| {n_q}/{n_kv} | {cache} | {Tq} | "
                        f"{tf[64]:.1f} (±{spread[64]:.0f}%) | "
                        f"{tf[128]:.1f} (±{spread[128]:.0f}%, {route}) | "
                        f"{tf[64] / tf[128]:.2f} |")
                print(line, flush=True)
                lines.append(line)
                del routes, ring, keep


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the markdown tables here")
    ap.add_argument("--quick", action="store_true",
                    help="decode B = 64 only, prefill Tq 512 and 2048 only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_hd64 needs a GPU"
    torch.manual_seed(0)
    lines = []
    bench_decode(lines, args.quick)
    bench_prefill(lines, args.quick)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
