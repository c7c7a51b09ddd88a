"""Attention kernels against the fp64 oracle, path by path.

Every case (1) asserts the launch plan it was written for through
``_C.prefill_plan`` / ``_C.decode_plan`` — the functions the launchers
themselves call — so a retuned host heuristic fails here instead of
silently moving coverage, and (2) holds the kernel to the derived
per-element bound of ``attention_oracle`` (derivation in its docstring):

    |kernel - out| <= 2**-7 * A + 2**-8 * |out| + 1e-6

on ``randn`` and on the structured ramp / needle inputs, over shuffled
block tables. The bound is derived, not tuned; no case family carries an
exception (worst measured err/bound per family: docs/kernels.md).
"""
import pytest
import torch

import kubeai_amd.ops as ops
from attention_oracle import (
    FAMILIES,
    assert_within_bound,
    make_case,
    oracle_decode,
    oracle_prefill,
)

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, E5M2 = torch.bfloat16, torch.float8_e5m2
DTYPES = [pytest.param(BF16, id="bf16"), pytest.param(E5M2, id="e5m2")]


def _C():
    assert ops.have_hip_ext()
    return ops._C


def _run_prefill(c, window=0, softcap=0.0):
    return ops.paged_attention_prefill(
        c["q"], c["k_cache"], c["v_cache"], c["block_tables"],
        c["query_start_loc"], c["seq_lens"], c["scale"], window=window,
        softcap=softcap)


def _run_decode(c, window=0, softcap=0.0):
    return ops.paged_attention_decode(
        c["q"], c["k_cache"], c["v_cache"], c["block_tables"], c["seq_lens"],
        c["scale"], window=window, softcap=softcap)


def _prefill_plan(c, window=0, softcap=0.0):
    q, kc, bt = c["q"], c["k_cache"], c["block_tables"]
    return _C().prefill_plan(q.shape[0], c["seq_lens"].shape[0], q.shape[1],
                             kc.shape[1], q.shape[2], bt.shape[1], window,
                             softcap)


def _decode_plan(c):
    return _C().decode_plan(c["q"].shape[0], c["k_cache"].shape[1],
                            c["block_tables"].shape[1])


def _check_prefill(c, plan, label, window=0, softcap=0.0):
    assert _prefill_plan(c, window, softcap) == plan
    got = _run_prefill(c, window, softcap)
    out, a = oracle_prefill(c["q"], c["k_cache"], c["v_cache"],
                            c["block_tables"], c["query_start_loc"],
                            c["seq_lens"], c["scale"], window, softcap)
    assert_within_bound(got, out, a, label)


def _check_decode(c, n_splits, label, window=0, softcap=0.0):
    assert _decode_plan(c) == n_splits
    got = _run_decode(c, window, softcap)
    out, a = oracle_decode(c["q"], c["k_cache"], c["v_cache"],
                           c["block_tables"], c["seq_lens"], c["scale"],
                           window, softcap)
    assert_within_bound(got, out, a, label)


# ---------------------------------------------------------------------------
# plans: the boundaries of the two host heuristics themselves
# ---------------------------------------------------------------------------

def test_plan_functions():
    C = _C()
    # v1 <-> v2: single-sequence small-q continuation, approx_L > 3 * Tq
    assert C.prefill_plan(200, 1, 8, 2, 128, 37) == (2, 4)   # 592 <= 600
    assert C.prefill_plan(200, 1, 8, 2, 128, 38) == (1, 4)   # 608 > 600
    assert C.prefill_plan(1025, 1, 32, 8, 128, 4096) == (2, 4)  # Tq > 1024
    assert C.prefill_plan(1024, 1, 32, 8, 128, 1024) == (1, 4)  # 16k ctx
    assert C.prefill_plan(200, 2, 8, 2, 128, 38) == (2, 4)   # B > 1
    # window / softcap / hd 256 / odd group sizes run v1, G waves
    assert C.prefill_plan(200, 2, 8, 2, 128, 38, 48, 0.0) == (1, 4)
    assert C.prefill_plan(200, 2, 8, 2, 128, 38, 0, 50.0) == (1, 4)
    assert C.prefill_plan(200, 2, 8, 4, 256, 38) == (1, 2)
    # 4 <-> 8 waves: B * n_kv * ceil(Tq / ((8 / G) * 32)) >= 256
    assert C.prefill_plan(256, 8, 32, 8, 128, 30) == (2, 8)   # 8*8*4
    assert C.prefill_plan(192, 8, 32, 8, 128, 30) == (2, 4)   # 8*8*3
    assert C.prefill_plan(256, 8, 32, 32, 128, 30) == (2, 8)  # G=1: 8*32*1
    assert C.prefill_plan(256, 8, 31, 31, 128, 30) == (2, 4)
    assert C.prefill_plan(16, 1, 32, 4, 128, 1) == (2, 8)     # G=8: always
    # decode: ceil(2048 / (B * n_kv)) capped at 16, 1 from 2048 workgroups
    assert C.decode_plan(257, 1, 17) == 8
    assert C.decode_plan(128, 1, 17) == 16
    assert C.decode_plan(129, 1, 17) == 16
    assert C.decode_plan(137, 1, 17) == 15
    assert C.decode_plan(256, 4, 3) == 2
    assert C.decode_plan(2047, 1, 3) == 2
    assert C.decode_plan(256, 8, 3) == 1


# ---------------------------------------------------------------------------
# prefill v2 (hd 128, no window, no softcap)
# ---------------------------------------------------------------------------

_RAGGED_Q = [37, 64, 5, 1, 33, 20, 17, 26]     # 203 query tokens
_RAGGED_CTX = [0, 300, 0, 100, 16, 0, 91, 0]   # seq 1: L = 364, 6 KV tiles

# id -> (q_lens, ctx_lens, n_q, n_kv, plan)
_V2_CASES = {
    # 4-wave form: B * n_kv * ceil(103 / qrows8) << 256
    "w4-G1": ([70, 33], [0, 150], 2, 2, (2, 4)),
    "w4-G2": ([70, 33], [0, 150], 4, 2, (2, 4)),
    "w4-G4": ([70, 33], [0, 150], 8, 2, (2, 4)),
    # 8-wave form: 8 * n_kv * ceil(203 / ((8/G) * 32)) == 256
    "w8-G1": (_RAGGED_Q, _RAGGED_CTX, 32, 32, (2, 8)),
    "w8-G2": (_RAGGED_Q, _RAGGED_CTX, 32, 16, (2, 8)),
    "w8-G4": (_RAGGED_Q, _RAGGED_CTX, 32, 8, (2, 8)),
    # G = 8 has the 8-wave form only (one 32-row subtile per head)
    "w8-G8": (_RAGGED_Q, _RAGGED_CTX, 32, 4, (2, 8)),
    # one sequence, 8 KV tiles, table 32 blocks wide: 512 <= 3 * 200 keeps
    # it on v2; early waves see interior tiles, late ones the diagonal, and
    # the double buffer wraps three times
    "multi-tile": ([200], [300], 8, 2, (2, 4)),
}


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("cache_dtype", DTYPES)
@pytest.mark.parametrize("case", list(_V2_CASES))
def test_prefill_v2(case, cache_dtype, family):
    q_lens, ctx, n_q, n_kv, plan = _V2_CASES[case]
    c = make_case(family, q_lens, ctx, n_q, n_kv, cache_dtype=cache_dtype,
                  device=DEV, seed=11)
    _check_prefill(c, plan, f"prefill_v2/{case}/{family}")


# ---------------------------------------------------------------------------
# prefill v1
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("cache_dtype", DTYPES)
def test_prefill_v1_small_q_continuation(cache_dtype, family):
    """[32] new tokens against 480 cached: 512 > 3 * 32 routes to v1."""
    c = make_case(family, [32], [480], 8, 2, cache_dtype=cache_dtype,
                  device=DEV, seed=12)
    _check_prefill(c, (1, 4), f"prefill_v1/continuation/{family}")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("cache_dtype", DTYPES)
@pytest.mark.parametrize("window", [48, 17])
def test_prefill_v1_window(window, cache_dtype, family):
    """Window edges at both ramps: ramp_down puts the mass on key
    p - window + 1, ramp_up on key p; 17 is no multiple of anything."""
    c = make_case(family, [120, 40, 33], [0, 60, 300], 8, 2,
                  cache_dtype=cache_dtype, device=DEV, seed=13)
    _check_prefill(c, (1, 4), f"prefill_v1/window/{family}", window=window)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("cache_dtype", DTYPES)
@pytest.mark.parametrize("window", [0, 48])
def test_prefill_v1_hd256_softcap(window, cache_dtype, family):
    c = make_case(family, [64, 17, 40], [30, 50, 0], 8, 4, hd=256,
                  cache_dtype=cache_dtype, device=DEV, seed=14)
    _check_prefill(c, (1, 2), f"prefill_v1/hd256/{family}", window=window,
                   softcap=50.0)


@pytest.mark.parametrize("n_q,n_kv", [(8, 8), (16, 2)])
def test_prefill_v1_group_sizes(n_q, n_kv):
    """G = 1 and G = 8 through v1 (window forces it)."""
    c = make_case("ramp_down", [70, 33], [0, 150], n_q, n_kv, device=DEV,
                  seed=15)
    _check_prefill(c, (1, n_q // n_kv), f"prefill_v1/G{n_q // n_kv}/ramp_down",
                   window=48)


# ---------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------

# 1, 16, 17: one token, exactly one block, one block + one token
_DEC_LENS = [257, 64, 19, 100, 1, 16, 17]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("cache_dtype", DTYPES)
@pytest.mark.parametrize("G", [1, 4, 8])
@pytest.mark.parametrize("hd", [128, 256])
def test_decode(hd, G, cache_dtype, family):
    """16 splits over at most 17 blocks: chunks of 2 blocks, one per wave,
    trailing splits empty; short sequences leave most splits empty."""
    B = len(_DEC_LENS)
    c = make_case(family, [1] * B, [L - 1 for L in _DEC_LENS], 2 * G, 2,
                  hd=hd, cache_dtype=cache_dtype, device=DEV, seed=21)
    _check_decode(c, 16, f"decode/hd{hd}/G{G}/{family}")


@pytest.mark.parametrize("cache_dtype", DTYPES)
@pytest.mark.parametrize("G", [2, 5, 6])
@pytest.mark.parametrize("hd", [128, 256])
def test_decode_other_group_sizes(hd, G, cache_dtype):
    """The remaining instantiated group sizes (test_decode and the hd 256
    cases cover 1, 4, 8 and G = 2 at hd 256): a launcher that routed one of
    them to a neighbouring instantiation would read the wrong heads."""
    B = len(_DEC_LENS)
    c = make_case("randn", [1] * B, [L - 1 for L in _DEC_LENS], 2 * G, 2,
                  hd=hd, cache_dtype=cache_dtype, device=DEV, seed=21)
    _check_decode(c, 16, f"decode/hd{hd}/G{G}/randn")


def test_decode_rejects_unsupported_group_size():
    """G = 3 has no instantiation: a host error before any launch."""
    c = make_case("randn", [1], [16], 3, 1, device=DEV, seed=27)
    with pytest.raises(RuntimeError, match="unsupported GQA group size"):
        _run_decode(c)


@pytest.mark.parametrize("cache_dtype", DTYPES)
@pytest.mark.parametrize("hd", [128, 256])
def test_decode_window_ramp_down(hd, cache_dtype):
    """Window 48 with the mass on key L - 48; L = 48 and 49 straddle the
    first masked key, 257 starts the window inside block 13."""
    lens = [257, 64, 19, 100, 48, 49, 300]
    c = make_case("ramp_down", [1] * len(lens), [L - 1 for L in lens], 8, 2,
                  hd=hd, cache_dtype=cache_dtype, device=DEV, seed=22)
    _check_decode(c, 16, f"decode/hd{hd}/window/ramp_down", window=48)


@pytest.mark.parametrize("family", ["randn", "ramp_up"])
def test_decode_hd256_softcap(family):
    lens = [257, 64, 19]
    c = make_case(family, [1] * len(lens), [L - 1 for L in lens], 8, 4,
                  hd=256, device=DEV, seed=23)
    _check_decode(c, 16, f"decode/hd256/softcap/{family}", softcap=50.0)


@pytest.mark.parametrize("family", FAMILIES)
def test_decode_single_split(family):
    """B * n_kv = 2048 workgroups: no splits, the kernel normalises and
    writes bf16 itself (no merge launch)."""
    B = 256
    lens = [1 + (7 * i) % 45 for i in range(B)]
    c = make_case(family, [1] * B, [L - 1 for L in lens], 8, 8, device=DEV,
                  seed=24)
    _check_decode(c, 1, f"decode/single_split/{family}")


@pytest.mark.parametrize("cache_dtype", DTYPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_decode_graph_padded_batch(family, cache_dtype):
    """The shape of a graph-padded batch: tables padded with block 0 to 4x
    the needed width, two seq_len = 1 pad rows pointing at block 0. The
    wider table also moves the row stride away from the needed width."""
    B = len(_DEC_LENS)
    c = make_case(family, [1] * B, [L - 1 for L in _DEC_LENS], 8, 2,
                  cache_dtype=cache_dtype, device=DEV, seed=25, table_pad=4,
                  pad_rows=2)
    bt = c["block_tables"]
    assert bt.shape == (B + 2, 4 * 17)
    assert int(bt.min()) >= 0 and int(bt.max()) < c["k_cache"].shape[0]
    assert c["seq_lens"][-2:].tolist() == [1, 1]
    _check_decode(c, 16, f"decode/graph_padded/{family}")


def _needle_case(positions, cache_dtype):
    n = len(positions)
    return make_case("needle", [1] * n, [256] * n, 4, 1,
                     cache_dtype=cache_dtype, device=DEV, seed=26,
                     needle_pos=positions)


@pytest.mark.parametrize("cache_dtype", DTYPES)
def test_decode_needle_sweep_8_splits(cache_dtype):
    """L = 257, one sequence per needle position 0..256; 257 workgroups
    give 8 splits of 3 blocks (the last two empty)."""
    c = _needle_case(list(range(257)), cache_dtype)
    _check_decode(c, 8, "decode/needle/8_splits")
    # the needle really dominates: out ~ V[p]
    got = _run_decode(c)
    p = torch.arange(257, device=DEV)
    blk = c["block_tables"][p, p // 16].long()
    v_p = c["v_cache"].float()[blk, 0, p % 16]          # [257, hd]
    assert float((got.float() - v_p.unsqueeze(1)).abs().max()) < 0.25


@pytest.mark.parametrize("cache_dtype", DTYPES)
@pytest.mark.parametrize("lo,hi", [(0, 86), (86, 172), (172, 257)])
def test_decode_needle_sweep_16_splits(lo, hi, cache_dtype):
    """The same sweep in batches small enough for 16 splits: chunks of 2
    blocks, 9 splits used, 7 trailing ones empty."""
    c = _needle_case(list(range(lo, hi)), cache_dtype)
    _check_decode(c, 16, "decode/needle/16_splits")


# ---------------------------------------------------------------------------
# row-strided q into prefill
# ---------------------------------------------------------------------------

@pytest.mark.parametrize(
    "q_lens,ctx,window,plan",
    [([70, 33], [0, 150], 0, (2, 4)),
     (_RAGGED_Q, _RAGGED_CTX, 0, (2, 8)),
     ([70, 33], [0, 150], 48, (1, 4)),
     ([32], [480], 0, (1, 4))],
    ids=["v2-w4", "v2-w8", "v1-window", "v1-continuation"])
def test_prefill_strided_q(q_lens, ctx, window, plan):
    """q as a view into the fused [T, (n_q + 2 n_kv) * hd] qkv buffer must
    give the bits of the contiguous call."""
    n_q, n_kv, hd = 32, 8, 128
    c = make_case("randn", q_lens, ctx, n_q, n_kv, device=DEV, seed=31)
    assert _prefill_plan(c, window) == plan
    T = c["q"].shape[0]
    qkv = torch.randn(T, (n_q + 2 * n_kv) * hd, dtype=BF16, device=DEV)
    q_view = qkv[:, : n_q * hd].unflatten(-1, (n_q, hd))
    q_view.copy_(c["q"])
    assert not q_view.is_contiguous() and q_view.stride(0) != n_q * hd
    want = _run_prefill(c, window)
    got = _run_prefill(dict(c, q=q_view), window)
    assert torch.equal(got, want)
    out, a = oracle_prefill(c["q"], c["k_cache"], c["v_cache"],
                            c["block_tables"], c["query_start_loc"],
                            c["seq_lens"], c["scale"], window)
    assert_within_bound(got, out, a, "prefill/strided_q")
