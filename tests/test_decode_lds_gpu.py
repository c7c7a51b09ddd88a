"""paged_decode_kernel with one LDS tile buffer per wave against the bytes the
double-buffered kernel of the parent commit produced.

The change has no unfused twin in the tree, so the reference is a recording:
scripts/record_decode_golden.py ran the parent build on the inputs of
tests/decode_golden_cases.py and wrote `out`, the fp8 bytes, the row scales
and the new cache rows to tests/golden/decode_parent/. The same inputs go
through the current build here, and every byte has to match.

What a case reaches (block size 16, 2 waves per workgroup, every case plans
16 splits, asserted):
  L = 1, 16, 17   the new row is the whole context / the last row of a block
                  / the first row of the next one: the RAW row patch lands in
                  the only tile, in its last row, in a second block's first
  L = 100, 257    7 and 17 blocks over 16 splits: one and two blocks per
                  split, one tile per wave, empty splits behind them
  L = 1100, 1030  five blocks per split: wave 0 stages three tiles into its
                  one buffer (overwritten twice), wave 1 two; at L = 1030 the
                  new row is patched into the third tile of wave 0
  e5m2 cache, hd 256 with softcap, window 48: the other element width, the
                  two-pass tile and the masked straddling block
"""
import os

import numpy as np
import pytest
import torch

import decode_golden_cases as cases
import kubeai_amd.ops as ops

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "decode_parent")

_INPUTS = {}


def _inputs(name):
    if name not in _INPUTS:
        _INPUTS[name] = cases.build_inputs(name, "cuda")
    return _INPUTS[name]


_PARAMS = [
    (name, raw, fp8_out)
    for name, c in cases.CASES.items()
    for raw, fp8_out in c["variants"]
]


@pytest.mark.parametrize(
    "name,raw,fp8_out", _PARAMS,
    ids=[f"{n}-{cases.variant_name(r, f)}" for n, r, f in _PARAMS],
)
def test_bytes_equal_parent(name, raw, fp8_out):
    c = cases.CASES[name]
    inp = _inputs(name)
    B, width = inp["block_tables"].shape
    assert ops._C.decode_plan(B, c["n_kv"], width) == cases.EXPECT_SPLITS
    kc0, vc0 = inp["k_cache"].clone(), inp["v_cache"].clone()

    sections, kc, vc = cases.run_variant(ops, inp, raw, fp8_out)
    golden = np.load(
        os.path.join(GOLDEN, f"{name}_{cases.variant_name(raw, fp8_out)}.npy")
    )
    assert golden.dtype == np.uint8
    assert golden.size == sum(s.size for s in sections.values())
    ofs = 0
    for sec, got in sections.items():
        want = golden[ofs : ofs + got.size]
        ofs += got.size
        diff = int((got != want).sum())
        assert diff == 0, f"{sec}: {diff} of {got.size} bytes differ"

    # the shared inputs are as they were, and the caches hold the new rows
    # and nothing else new
    u8 = lambda t: t.view(torch.uint8)
    assert torch.equal(u8(inp["k_cache"]), u8(kc0))
    assert torch.equal(u8(inp["v_cache"]), u8(vc0))
    if raw:
        s = inp["slots"]
        assert not torch.equal(u8(kc), u8(kc0))
        u8(kc0)[s // cases.BS, :, s % cases.BS, :] = cases.new_rows(kc, s)
        u8(vc0)[s // cases.BS, :, s % cases.BS, :] = cases.new_rows(vc, s)
    assert torch.equal(u8(kc), u8(kc0))
    assert torch.equal(u8(vc), u8(vc0))
