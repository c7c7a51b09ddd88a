"""rope_cache_attention_decode (rotary embedding and KV-cache write inside
the decode attention kernel) against the two-launch sequence it replaces,
rope_and_cache followed by paged_attention_decode: bit for bit in `out`, the
fp8 bytes, the row scales and every byte of both caches, with q, k and v left
untouched.

Where the new row can go wrong, and the case that reaches it (block size 16,
2 waves per workgroup, wave w of a split takes its blocks w, w+2, ...):
  L = 1     the new row is the whole context
  L = 16    last row of a block
  L = 17    first row of the next block (wave 1 of the split when
            n_splits == 1, the [17] * 256 case)
  L = 33, 100   with B <= 4 the plan is 16 splits of one block each: the
            owner is a different split per length and the splits past the
            last block are empty
  L = 300, 320  two blocks per split: the owner is wave 0 / wave 1 of the
            last non-empty split
"""
import math

import pytest
import torch

import kubeai_amd.ops as ops
from kubeai_amd.ops import ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
BS = 16


@pytest.fixture(autouse=True)
def _fused_on(monkeypatch):
    monkeypatch.delenv("KUBEAI_DECODE_ROPE_FUSED", raising=False)
    torch.manual_seed(97)


def _bytes(t):
    return t.view(torch.uint8) if t.dtype != torch.bfloat16 else t.view(torch.int16)


_CS = {}


def _cos_sin(hd):
    if hd not in _CS:
        _CS[hd] = ref.make_cos_sin_cache(hd, 4096, 500000.0).to(DEV)
    return _CS[hd]


def _check(
    nq, nkv, hd, lens, cache_dtype=torch.bfloat16, layout="qkv_views",
    window=0, softcap=0.0, pos=None, bt_width=None, pad_rows=(),
    expect_splits=None, fp8_out=True,
):
    """`pad_rows`: indices of `lens` that are graph pad rows (slot -1,
    seq_len 1, block table 0); their `lens` entry is ignored."""
    B = len(lens)
    lens = [1 if b in pad_rows else L for b, L in enumerate(lens)]
    n_blk = [(L + BS - 1) // BS for L in lens]
    width = bt_width or max(n_blk)
    # block 0 belongs to the pad rows; real sequences draw distinct blocks
    # from a shuffled pool so that neighbours in a table are not neighbours
    # in memory
    nb = 1 + sum(n_blk)
    pool = (torch.randperm(nb - 1) + 1).tolist()
    bt = torch.zeros(B, width, dtype=torch.int32)
    slots = []
    for b, L in enumerate(lens):
        if b in pad_rows:
            slots.append(-1)
            continue
        blocks = [pool.pop() for _ in range(n_blk[b])]
        bt[b, : n_blk[b]] = torch.tensor(blocks, dtype=torch.int32)
        slots.append(blocks[(L - 1) // BS] * BS + (L - 1) % BS)
    bt = bt.to(DEV)
    slots = torch.tensor(slots, dtype=torch.int64, device=DEV)
    seq_lens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    if pos is None:
        pos = [L - 1 for L in lens]
    pos = torch.tensor(pos, dtype=torch.int32, device=DEV)
    cs = _cos_sin(hd)
    scale = 1.0 / math.sqrt(hd)
    kc0 = torch.randn(nb, nkv, BS, hd, device=DEV).to(cache_dtype)
    vc0 = torch.randn(nb, nkv, BS, hd, device=DEV).to(cache_dtype)
    qkv0 = torch.randn(B, (nq + 2 * nkv) * hd, dtype=torch.bfloat16, device=DEV)

    if expect_splits is not None:
        assert ops._C.decode_plan(B, nkv, width) == expect_splits

    def split(buf):
        q, k, v = buf.split([nq * hd, nkv * hd, nkv * hd], dim=-1)
        q = q.unflatten(-1, (nq, hd))
        k = k.unflatten(-1, (nkv, hd))
        v = v.unflatten(-1, (nkv, hd))
        if layout == "separate":
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        return q, k, v

    # the two-launch sequence
    q_a, k_a, v_a = split(qkv0.clone())
    kc_a, vc_a = kc0.clone(), vc0.clone()
    ops.rope_and_cache(q_a, k_a, v_a, pos, cs, kc_a, vc_a, slots)
    res_a = ops.paged_attention_decode(
        q_a, kc_a, vc_a, bt, seq_lens, scale, window=window, softcap=softcap,
        fp8_out=fp8_out,
    )

    # fused
    q_b, k_b, v_b = split(qkv0.clone())
    kc_b, vc_b = kc0.clone(), vc0.clone()
    res_b = ops.rope_cache_attention_decode(
        q_b, k_b, v_b, pos, cs, kc_b, vc_b, slots, bt, seq_lens, scale,
        window=window, softcap=softcap, fp8_out=fp8_out,
    )

    if fp8_out:
        out_a, f8_a, sc_a = res_a
        out_b, f8_b, sc_b = res_b
        assert f8_b.shape == (B, nq * hd) and sc_b.shape == (B,)
        assert torch.equal(f8_b.view(torch.uint8), f8_a.view(torch.uint8))
        assert torch.equal(sc_b, sc_a)
    else:
        out_a, out_b = res_a, res_b
    assert torch.equal(out_b, out_a)
    assert torch.equal(_bytes(kc_b), _bytes(kc_a))
    assert torch.equal(_bytes(vc_b), _bytes(vc_a))
    # the caches did change; q, k and v did not (the two-launch sequence
    # rotated its q and k in place)
    if len(pad_rows) < B:
        assert not torch.equal(_bytes(kc_b), _bytes(kc0))
        assert not torch.equal(_bytes(vc_b), _bytes(vc0))
    q_0, k_0, v_0 = split(qkv0)
    assert torch.equal(q_b, q_0) and torch.equal(k_b, k_0)
    assert torch.equal(v_b, v_0)
    if bool((pos != 0).any()):  # position 0 is the identity rotation
        assert not torch.equal(q_a, q_0)
    # pad rows leave block 0 as it was
    assert torch.equal(_bytes(kc_b[0]), _bytes(kc0[0]))
    assert torch.equal(_bytes(vc_b[0]), _bytes(vc0[0]))
    return out_b


# G = 4, 8, 1, 2, then the other instantiated group sizes: 2 at hd 128, 5, 6
HEADS = [(32, 8, 128), (8, 1, 128), (8, 8, 128), (8, 4, 256),
         (4, 2, 128), (10, 2, 128), (12, 2, 256)]


@pytest.mark.parametrize("cache_dtype", [torch.bfloat16, torch.float8_e5m2])
@pytest.mark.parametrize("layout", ["qkv_views", "separate"])
@pytest.mark.parametrize("lens", [[1, 16, 17, 33], [100, 33, 17]])
@pytest.mark.parametrize("nq,nkv,hd", HEADS)
def test_fused_equals_two_launches(nq, nkv, hd, lens, layout, cache_dtype):
    _check(nq, nkv, hd, lens, cache_dtype=cache_dtype, layout=layout,
           expect_splits=16)


@pytest.mark.parametrize("cache_dtype", [torch.bfloat16, torch.float8_e5m2])
def test_two_blocks_per_split(cache_dtype):
    # 19 and 20 blocks over 16 splits: chunk 2, the new row's block is the
    # first (wave 0) resp. the second (wave 1) block of split 9
    _check(32, 8, 128, [300, 320], cache_dtype=cache_dtype, expect_splits=16)


# B * n_kv = 2048 workgroups: one split, no merge launch; with [17] * 256
# block 1 of every sequence belongs to wave 1. 256 rows are also ~10^6
# rotated q elements: a rotation that contracts its multiply-adds another
# way than rope_and_cache is one bf16 ulp off in about one element in 10^5
# (it was, until rope_rotate_pair spelled its fma), which the 4-row cases
# above are too small to see.
@pytest.mark.parametrize("cache_dtype", [torch.bfloat16, torch.float8_e5m2])
@pytest.mark.parametrize("lens", [[17] * 256, [16, 33, 1, 100] * 64])
def test_single_split(lens, cache_dtype):
    _check(32, 8, 128, lens, cache_dtype=cache_dtype, expect_splits=1)


def test_bf16_out_only():
    _check(32, 8, 128, [100, 33, 17], fp8_out=False)
    _check(32, 8, 128, [17] * 256, fp8_out=False, expect_splits=1)


def test_window():
    _check(32, 8, 128, [100, 37], window=48)


@pytest.mark.parametrize("cache_dtype", [torch.bfloat16, torch.float8_e5m2])
def test_hd256_softcap(cache_dtype):
    _check(8, 4, 256, [100, 33, 17, 1], softcap=50.0, window=40,
           cache_dtype=cache_dtype)


@pytest.mark.parametrize("cache_dtype", [torch.bfloat16, torch.float8_e5m2])
def test_pad_row(cache_dtype):
    # row 1 is a graph pad row: slot -1, seq_len 1, block table 0
    _check(32, 8, 128, [33, 0, 17], pad_rows=(1,), cache_dtype=cache_dtype)


def test_all_pad_rows():
    # what graph warm-up and capture run: nothing may be written
    _check(32, 8, 128, [0, 0], pad_rows=(0, 1))


def test_angle_comes_from_positions():
    lens = [100, 33, 17]
    torch.manual_seed(5)
    a = _check(32, 8, 128, lens)
    torch.manual_seed(5)
    b = _check(32, 8, 128, lens, pos=[7, 2000, 311])
    assert not torch.equal(a, b)


def test_wide_block_table():
    # the graph path's table width: the plan follows the width, not the
    # lengths (40 rows of 512 blocks -> 7 splits, mostly empty here)
    lens = [100, 17, 33, 1] * 10
    _check(32, 8, 128, lens, bt_width=512, expect_splits=7)


def test_switch_restores_two_launches(monkeypatch):
    # KUBEAI_DECODE_ROPE_FUSED=0: rope_and_cache runs again, so q and k are
    # rotated in place; results are those of the fused call
    nq, nkv, hd, L = 32, 8, 128, 40
    cs = _cos_sin(hd)
    bt = torch.tensor([[1, 2, 3]], dtype=torch.int32, device=DEV)
    seq_lens = torch.tensor([L], dtype=torch.int32, device=DEV)
    pos = torch.tensor([L - 1], dtype=torch.int32, device=DEV)
    slots = torch.tensor([3 * BS + (L - 1) % BS], dtype=torch.int64, device=DEV)
    kc0 = torch.randn(4, nkv, BS, hd, dtype=torch.bfloat16, device=DEV)
    vc0 = torch.randn(4, nkv, BS, hd, dtype=torch.bfloat16, device=DEV)
    q0 = torch.randn(1, nq, hd, dtype=torch.bfloat16, device=DEV)
    k0 = torch.randn(1, nkv, hd, dtype=torch.bfloat16, device=DEV)
    v0 = torch.randn(1, nkv, hd, dtype=torch.bfloat16, device=DEV)
    res = []
    for flag in ("1", "0"):
        monkeypatch.setenv("KUBEAI_DECODE_ROPE_FUSED", flag)
        q, k, kc, vc = q0.clone(), k0.clone(), kc0.clone(), vc0.clone()
        out = ops.rope_cache_attention_decode(
            q, k, v0, pos, cs, kc, vc, slots, bt, seq_lens, 1.0 / math.sqrt(hd)
        )
        res.append((out, kc, vc))
        assert torch.equal(q, q0) == (flag == "1")
    assert all(torch.equal(a, b) for a, b in zip(*res))


def test_engine_tokens_and_logprobs(monkeypatch):
    """llama-tiny fp8, 12 greedy tokens: the switch changes launches, not
    one token or logprob."""
    from kubeai_amd.engine import EngineConfig, LLMEngine, SamplingParams

    runs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("KUBEAI_DECODE_ROPE_FUSED", flag)
        eng = LLMEngine(
            EngineConfig(
                model="llama-tiny", device="cuda", max_model_len=512,
                num_gpu_blocks=256, seed=0, quantization="fp8",
            )
        )
        eng.add_request(
            list(range(10, 140)), SamplingParams(max_tokens=12), request_id="r"
        )
        toks, lps = [], []
        for _ in range(64):
            if not eng.has_work():
                break
            for o in eng.step():
                toks.extend(o.new_token_ids)
                lps.append(o.logprob)
        assert not eng.has_work()
        runs.append((toks, lps))
    assert len(runs[0][0]) == 12
    assert runs[0] == runs[1]
