"""paged_attention_append (attention_append.hip) against the fp64 oracle.

The bound is attention_oracle's, unchanged:

    |kernel - out| <= 2**-7 * A + 2**-8 * |out| + 1e-6

P is rounded to bf16 before PV, l is summed from the unrounded p, the output
is rounded to bf16 once; the fp32 split merge is orders below those terms.
"""
import functools

import pytest
import torch

import kubeai_amd.ops as ops
from attention_oracle import assert_within_bound, make_case, oracle_prefill

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, E5M2 = torch.bfloat16, torch.float8_e5m2
DTYPES = {"bf16": BF16, "e5m2": E5M2}

# 16 | 17 is a q-tile boundary; ctx 0 is all diagonal; 15 / 300 / 100 end
# inside a block and a 32-key tile; rows 16..31 of the last sequence sit at
# positions 506..521, so the key tile starting at 512 is a split of its own
# at 16 splits and holds no visible key for the rows below it
Q_LENS = [1, 5, 16, 17, 33]
CTX_LENS = [0, 15, 300, 100, 490]
N_KV = 2


@functools.lru_cache(maxsize=None)
def _case(family, G, cache):
    c = make_case(family, Q_LENS, CTX_LENS, N_KV * G, N_KV,
                  cache_dtype=DTYPES[cache], device=DEV)
    out, a = oracle_prefill(c["q"], c["k_cache"], c["v_cache"],
                            c["block_tables"], c["query_start_loc"],
                            c["seq_lens"], c["scale"])
    return c, out, a


def _append(c, q=None, **kw):
    return ops.paged_attention_append(
        c["q"] if q is None else q, c["k_cache"], c["v_cache"],
        c["block_tables"], c["query_start_loc"], c["seq_lens"], c["scale"],
        **kw)


# n_splits 1: no merge; 3: ragged ranges; 16: both merge tiers and the
# trailing empty splits of the short sequences
_RANDN = [("randn", G, cache, s) for G in (1, 2, 4, 8)
          for cache in ("bf16", "e5m2") for s in (1, 3, 16)]
_RAMPS = [(family, G, cache, s)
          for family in ("ramp_up", "ramp_down")
          for G, cache, s in [(1, "bf16", 16), (2, "e5m2", 3), (4, "bf16", 1),
                              (4, "e5m2", 16), (8, "e5m2", 1),
                              (8, "bf16", 3)]]


@pytest.mark.parametrize("family,G,cache,n_splits", _RANDN + _RAMPS)
def test_append_oracle_bound(family, G, cache, n_splits):
    c, out, a = _case(family, G, cache)
    got = _append(c, n_splits=n_splits)
    assert_within_bound(got, out, a,
                        f"append {family} G{G} {cache} S{n_splits}")


@pytest.mark.parametrize("n_splits", [1, 16])
def test_append_strided_q_and_rerun(n_splits):
    c, _, _ = _case("randn", 4, "bf16")
    q = c["q"]
    Tq, n_q, hd = q.shape
    qkv = torch.randn(Tq, (n_q + 2 * N_KV) * hd, device=DEV).to(BF16)
    q_view = qkv[:, :n_q * hd].view(Tq, n_q, hd)
    q_view.copy_(q)
    assert not q_view.is_contiguous()
    want = _append(c, n_splits=n_splits)
    assert torch.equal(_append(c, q=q_view, n_splits=n_splits), want)
    assert torch.equal(_append(c, n_splits=n_splits), want)


def test_append_host_errors():
    c, _, _ = _case("randn", 1, "bf16")
    with pytest.raises(RuntimeError):
        _append(c, window=48)
    with pytest.raises(RuntimeError):
        _append(c, softcap=50.0)
    with pytest.raises(RuntimeError):
        _append(c, n_splits=17)
    g3 = make_case("randn", [5], [40], 3, 1, device=DEV)
    with pytest.raises(RuntimeError):
        _append(g3)
    hd256 = make_case("randn", [5], [40], 2, 1, hd=256, device=DEV)
    with pytest.raises(RuntimeError):
        _append(hd256)
    torch.cuda.synchronize()


def test_append_plan_thresholds():
    plan = ops._C.append_plan
    # (Tq, B, n_q, n_kv, hd, max_blocks[, window, softcap]) -> (taken, splits)
    # context: max_blocks * 16 >= kAppendMinCtx = 1024
    assert plan(20, 1, 32, 8, 128, 64) == (True, 16)
    assert plan(20, 1, 32, 8, 128, 63)[0] is False
    # underfill: B * n_kv * ceil(Tq / 16) < 256
    assert plan(16, 31, 32, 8, 128, 64)[0] is True      # 248
    assert plan(16, 32, 32, 8, 128, 64)[0] is False     # 256
    assert plan(17, 16, 32, 8, 128, 64)[0] is False     # 16 * 8 * 2
    # scope
    assert plan(20, 1, 32, 8, 256, 64)[0] is False
    assert plan(20, 1, 32, 8, 128, 64, 48, 0.0)[0] is False
    assert plan(20, 1, 32, 8, 128, 64, 0, 50.0)[0] is False
    assert plan(20, 1, 24, 8, 128, 64)[0] is False      # G = 3
    # splits: min(16, ceil(2048 / wgs)), 1 from 2048 workgroups, and at
    # most ceil(max_blocks / 2)
    assert plan(16, 16, 32, 8, 128, 64)[1] == 16        # 128 wgs
    assert plan(16, 17, 32, 8, 128, 64)[1] == 16        # 136 wgs: 15.06
    assert plan(16, 18, 32, 8, 128, 64)[1] == 15        # 144 wgs: 14.2
    assert plan(16, 31, 32, 8, 128, 64)[1] == 9         # 248 wgs
    assert plan(128, 31, 32, 8, 128, 64)[1] == 2        # 1984 wgs
    assert plan(128, 32, 32, 8, 128, 64)[1] == 1        # 2048 wgs
    assert plan(20, 1, 32, 8, 128, 7)[1] == 4
    assert plan(20, 1, 32, 8, 128, 1)[1] == 1


def test_append_routing(monkeypatch):
    # the smallest taken shape: one sequence, one kv head, 64 blocks
    c = make_case("randn", [20], [1004], 4, 1, device=DEV)
    args = (c["q"], c["k_cache"], c["v_cache"], c["block_tables"],
            c["query_start_loc"], c["seq_lens"], c["scale"])
    assert ops._C.append_plan(20, 1, 4, 1, 128, 64)[0] is True
    monkeypatch.setenv("KUBEAI_APPEND_ATTN", "1")
    assert torch.equal(ops.paged_attention_prefill(*args),
                       ops.paged_attention_append(*args))
    monkeypatch.delenv("KUBEAI_APPEND_ATTN")
    want = torch.empty_like(c["q"])
    ops._C.paged_attention_prefill(want, *args, 0, 0.0)
    assert torch.equal(ops.paged_attention_prefill(*args), want)
