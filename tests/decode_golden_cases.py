"""Inputs and result packing shared by scripts/record_decode_golden.py (which
records what a build of the decode attention kernel computes) and
tests/test_decode_lds_gpu.py (which compares the current build with the
recording in tests/golden/decode_parent/).

Inputs come from a seeded CPU generator, so both sides see the same bytes.
A case runs in up to four variants: "plain" is paged_attention_decode on the
caches as generated, "raw" is rope_cache_attention_decode (the kernel rotates
q and k and writes the new K/V row); each with and without the fp8 output.
One variant's results are packed into one uint8 array:
    out (bf16) | fp8 bytes | row scales (fp32) | new K rows | new V rows
with the sections a variant does not have left out (no fp8 output; "plain"
writes no cache row).
"""
import math

import numpy as np
import torch

BS = 16

# lens, n_kv, G, hd, cache dtype, window, softcap, variants (raw, fp8_out)
_ALL = [(False, False), (False, True), (True, False), (True, True)]
_TWO = [(False, True), (True, True)]
_LENS = [1, 16, 17, 100, 257]
CASES = {
    "c1_bf16": dict(lens=_LENS, n_kv=2, G=4, hd=128, cache=torch.bfloat16,
                    window=0, softcap=0.0, variants=_ALL),
    "c2_e5m2": dict(lens=_LENS[:3], n_kv=1, G=8, hd=128,
                    cache=torch.float8_e5m2, window=0, softcap=0.0,
                    variants=_TWO),
    "c3_hd256_cap": dict(lens=_LENS[:3], n_kv=2, G=2, hd=256,
                         cache=torch.bfloat16, window=0, softcap=50.0,
                         variants=_TWO),
    "c4_window": dict(lens=_LENS, n_kv=2, G=4, hd=128, cache=torch.bfloat16,
                      window=48, softcap=0.0, variants=_ALL),
    # B * n_kv < 128 always plans 16 splits, so a wave of the cases above
    # sees one tile. 65 and 69 blocks are 5 per split: wave 0 of a split
    # stages three tiles into its one buffer, wave 1 two. L = 1030 puts the
    # new row into block 64, the third tile of wave 0 of split 12.
    "c5_three_tiles": dict(lens=[1100, 1030], n_kv=2, G=4, hd=128,
                           cache=torch.bfloat16, window=0, softcap=0.0,
                           variants=[(False, False), (True, True)]),
}
EXPECT_SPLITS = 16


def variant_name(raw: bool, fp8_out: bool) -> str:
    return ("raw" if raw else "plain") + ("_fp8" if fp8_out else "")


def build_inputs(name: str, device: str) -> dict:
    c = CASES[name]
    g = torch.Generator().manual_seed(20240 + sorted(CASES).index(name))
    lens, n_kv, hd = c["lens"], c["n_kv"], c["hd"]
    n_q = n_kv * c["G"]
    B = len(lens)
    n_blk = [(L + BS - 1) // BS for L in lens]
    nb = 1 + sum(n_blk)  # block 0 stays unused
    pool = (torch.randperm(nb - 1, generator=g) + 1).tolist()
    bt = torch.zeros(B, max(n_blk), dtype=torch.int32)
    slots = []
    for b, L in enumerate(lens):
        blocks = [pool.pop() for _ in range(n_blk[b])]
        bt[b, : n_blk[b]] = torch.tensor(blocks, dtype=torch.int32)
        slots.append(blocks[(L - 1) // BS] * BS + (L - 1) % BS)

    def rand(*shape):
        return torch.randn(*shape, generator=g)

    from kubeai_amd.ops import ref

    return dict(
        q=rand(B, n_q, hd).to(torch.bfloat16).to(device),
        k=rand(B, n_kv, hd).to(torch.bfloat16).to(device),
        v=rand(B, n_kv, hd).to(torch.bfloat16).to(device),
        k_cache=rand(nb, n_kv, BS, hd).to(c["cache"]).to(device),
        v_cache=rand(nb, n_kv, BS, hd).to(c["cache"]).to(device),
        block_tables=bt.to(device),
        seq_lens=torch.tensor(lens, dtype=torch.int32, device=device),
        positions=torch.tensor([L - 1 for L in lens], dtype=torch.int32,
                               device=device),
        slots=torch.tensor(slots, dtype=torch.int64, device=device),
        cos_sin=ref.make_cos_sin_cache(hd, 2048, 500000.0).to(device),
        scale=1.0 / math.sqrt(hd),
        window=c["window"],
        softcap=c["softcap"],
    )


def _u8(t: torch.Tensor) -> np.ndarray:
    t = t.contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    elif t.dtype in (torch.float8_e5m2, torch.float8_e4m3fn):
        t = t.view(torch.uint8)
    return t.cpu().numpy().reshape(-1).view(np.uint8)


def run_variant(ops, inp: dict, raw: bool, fp8_out: bool):
    """Runs one variant on clones of the caches. Returns (sections, k_cache,
    v_cache): sections is an ordered {name: uint8 array}, the caches are what
    the call left behind."""
    kc, vc = inp["k_cache"].clone(), inp["v_cache"].clone()
    kw = dict(window=inp["window"], softcap=inp["softcap"], fp8_out=fp8_out)
    if raw:
        res = ops.rope_cache_attention_decode(
            inp["q"], inp["k"], inp["v"], inp["positions"], inp["cos_sin"],
            kc, vc, inp["slots"], inp["block_tables"], inp["seq_lens"],
            inp["scale"], **kw,
        )
    else:
        res = ops.paged_attention_decode(
            inp["q"], kc, vc, inp["block_tables"], inp["seq_lens"],
            inp["scale"], **kw,
        )
    sections = {}
    if fp8_out:
        out, f8, sc = res
        sections["out"] = _u8(out)
        sections["fp8"] = _u8(f8)
        sections["scale"] = _u8(sc)
    else:
        sections["out"] = _u8(res)
    if raw:
        sections["k_rows"] = _u8(new_rows(kc, inp["slots"]))
        sections["v_rows"] = _u8(new_rows(vc, inp["slots"]))
    return sections, kc, vc


def new_rows(cache: torch.Tensor, slots: torch.Tensor) -> torch.Tensor:
    """The bytes of the cache rows at `slots`, [B, n_kv, row bytes] uint8."""
    return cache.view(torch.uint8)[slots // BS, :, slots % BS, :]


def pack(sections: dict) -> np.ndarray:
    return np.concatenate(list(sections.values()))
