"""CPU self-check of the attention checker (attention_oracle.py).

The GPU module trusts three things: the fp64 oracle, the derived bound and
the input families. Here the checker must

* ACCEPT the fp32 ``ops/ref.py`` result and a tilewise emulation of the
  kernel arithmetic (64-key tiles, a running maximum allowed to lag up to
  8, P rounded to bf16 before PV, ``l`` summed unrounded, bf16 output);
* REJECT kernels that are subtly wrong: causal bound +-1, window lower
  edge +-1, a dropped 16-token block, two swapped block-table entries, an
  online softmax that forgets to rescale ``o`` — each by at least one
  input family at every shape it applies to.
"""
import pytest
import torch

from attention_oracle import (
    BS,
    FAMILIES,
    accepts,
    gather_kv,
    make_case,
    oracle_decode,
    oracle_prefill,
    scores,
    worst_ratio,
)
from kubeai_amd.ops import ref

N_Q, N_KV, HD = 2, 1, 128
LENS = [96, 300]     # one sequence, every position a query row
WINDOWS = [0, 48]
SHAPES = [(L, w) for L in LENS for w in WINDOWS]


_cache = {}


def _case(family, L):
    """(case, fp64 q, whole-block fp64 K, V) — built once, never modified."""
    key = (family, L)
    if key not in _cache:
        c = make_case(family, [L], [0], N_Q, N_KV, HD, seed=5,
                      needle_pos=[L // 2 + 3])  # used by "needle" only
        n_pad = (L + BS - 1) // BS * BS
        k, v = gather_kv(c["k_cache"].double(), c["v_cache"].double(),
                         c["block_tables"][0], n_pad)
        _cache[key] = (c, c["q"].double(), k, v)
    return _cache[key]


def _oracle(family, L, window):
    key = (family, L, window, "oracle")
    if key not in _cache:
        c = _case(family, L)[0]
        _cache[key] = oracle_prefill(
            c["q"], c["k_cache"], c["v_cache"], c["block_tables"],
            c["query_start_loc"], c["seq_lens"], c["scale"], window)
    return _cache[key]


def _mask(L, n_keys, window, causal_shift=0, window_shift=0, drop_block=None):
    """[rows, keys] visibility of a (possibly wrong) kernel. Keys beyond L
    (the tail of the last block) are there to be wrongly read."""
    qpos = torch.arange(L).unsqueeze(1)
    kpos = torch.arange(n_keys).unsqueeze(0)
    good = kpos <= qpos
    vis = kpos <= qpos + causal_shift
    if window > 0:
        good = good & (kpos > qpos - window)
        vis = vis & (kpos > qpos - window + window_shift)
    if drop_block is not None:
        vis = vis & (kpos // BS != drop_block)
    empty = ~vis.any(1, keepdim=True)  # e.g. row 0 under causal - 1
    return torch.where(empty, good, vis)


def _swap_blocks(x, a, b):
    x = x.clone()
    x[a * BS:(a + 1) * BS], x[b * BS:(b + 1) * BS] = (
        x[b * BS:(b + 1) * BS].clone(), x[a * BS:(a + 1) * BS].clone())
    return x


def _exact(q, k, v, vis, scale):
    """fp64 attention under an arbitrary visibility mask."""
    s = scores(q, k, scale).masked_fill(~vis.unsqueeze(0), float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.einsum("hql,lhd->qhd", p,
                        v.repeat_interleave(q.shape[1] // v.shape[1], dim=1))


def _emulate(q, k, v, vis, scale, defer=True, rescale_o=True):
    """The kernels' arithmetic in fp32: 64-key tiles, online softmax with
    the defer-max shortcut (a row keeps its stale maximum while the tile's
    maximum is at most 8 above it), bf16 P into the PV product, fp32 l from
    the unrounded p, bf16 output. rescale_o=False is the mutant that never
    applies the correction to the accumulator."""
    g = q.shape[1] // k.shape[1]
    qf = q.float()
    kf = k.float().repeat_interleave(g, dim=1)
    vf = v.float().repeat_interleave(g, dim=1)
    s = torch.einsum("qhd,lhd->hql", qf, kf) * scale
    s = s.masked_fill(~vis.unsqueeze(0), float("-inf"))
    h, rows, keys = s.shape
    m = torch.full((h, rows), float("-inf"))
    l = torch.zeros(h, rows)
    o = torch.zeros(h, rows, q.shape[2])
    for t0 in range(0, keys, 64):
        st = s[..., t0:t0 + 64]
        pmax = st.max(-1).values
        keep = (pmax <= m + 8.0) if defer else (pmax <= m)
        m_new = torch.where(keep, m, torch.maximum(m, pmax))
        corr = torch.where(torch.isinf(m), torch.zeros_like(m),
                           torch.exp(m - m_new))
        corr = torch.where(keep, torch.ones_like(m), corr)
        l = l * corr
        if rescale_o:
            o = o * corr.unsqueeze(-1)
        p = torch.exp(st - m_new.unsqueeze(-1))
        p = torch.where(torch.isinf(st), torch.zeros_like(p), p)
        l = l + p.sum(-1)
        o = o + torch.einsum("hql,lhd->hqd", p.bfloat16().float(),
                             vf[t0:t0 + 64])
        m = m_new
    return (o / l.unsqueeze(-1)).bfloat16().transpose(0, 1)


# ---------------------------------------------------------------------------
# accepted
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("L,window", SHAPES)
@pytest.mark.parametrize("family", FAMILIES + ("needle",))
def test_accepts_fp32_reference(family, L, window):
    c = _case(family, L)[0]
    out, a = _oracle(family, L, window)
    got = ref.paged_attention_prefill(
        c["q"].float(), c["k_cache"].float(), c["v_cache"].float(),
        c["block_tables"], c["query_start_loc"], c["seq_lens"], c["scale"],
        window=window)
    assert got.dtype == torch.float32
    assert worst_ratio(got, out, a) < 0.05
    # and its bf16 rounding, what the existing GPU tests compare against
    assert worst_ratio(got.bfloat16(), out, a) <= 0.5


@pytest.mark.parametrize("defer", [True, False])
@pytest.mark.parametrize("L,window", SHAPES)
@pytest.mark.parametrize("family", FAMILIES + ("needle",))
def test_accepts_kernel_arithmetic(family, L, window, defer):
    c, q, k, v = _case(family, L)
    out, a = _oracle(family, L, window)
    got = _emulate(q, k, v, _mask(L, k.shape[0], window), c["scale"],
                   defer=defer)
    r = worst_ratio(got, out, a)
    # the bound is the derived first-order worst case doubled; the worst
    # here is 0.51 (ramp_up at L = 300, where fp32 scores of magnitude
    # ~260 add a 1e-4 relative error to p on top of the bf16 terms)
    print(f"emulation {family} L={L} window={window} defer={defer}: {r:.3f}")
    assert r <= 1.0, r


@pytest.mark.parametrize("cache_dtype", [torch.bfloat16, torch.float8_e5m2])
@pytest.mark.parametrize("L,window", SHAPES)
@pytest.mark.parametrize("family", FAMILIES + ("needle",))
def test_accepts_decode_reference(family, L, window, cache_dtype):
    """Decode form (one row per sequence), e5m2 cache included, against
    ref.paged_attention_decode; needle positions cross every block edge."""
    pos = sorted(set(range(0, L, 5)) | {15, 16, 17, L - 2, L - 1})
    n = len(pos)
    c = make_case(family, [1] * n, [L - 1] * n, 4, 2, HD,
                  cache_dtype=cache_dtype, seed=6, table_pad=2, pad_rows=1,
                  needle_pos=pos)
    out, a = oracle_decode(c["q"], c["k_cache"], c["v_cache"],
                           c["block_tables"], c["seq_lens"], c["scale"],
                           window)
    got = ref.paged_attention_decode(
        c["q"].float(), c["k_cache"].float(), c["v_cache"].float(),
        c["block_tables"], c["seq_lens"], c["scale"], window=window)
    assert worst_ratio(got, out, a) < 0.05
    if family == "needle":
        # needle dominates: out ~ V at the needle (inside the window only)
        for b, p in enumerate(pos):
            if window and p <= L - 1 - window:
                continue
            blk = int(c["block_tables"][b, p // BS])
            v_p = c["v_cache"].float()[blk, :, p % BS]      # [n_kv, hd]
            assert float((out[b, ::2] - v_p).abs().max()) < 0.1


def test_case_layout():
    """Shuffled, disjoint physical blocks; block 0 only as padding."""
    c = make_case("ramp_up", [1, 1, 1], [256, 18, 0], 4, 2, HD, seed=7,
                  table_pad=4, pad_rows=2)
    bt = c["block_tables"]
    assert bt.shape == (5, 4 * 17)
    assert c["seq_lens"].tolist() == [257, 19, 1, 1, 1]
    used = torch.cat([bt[0, :17], bt[1, :2], bt[2, :1]])
    assert sorted(used.tolist()) == list(range(1, 21))
    assert used.tolist() != sorted(used.tolist())  # not arange
    assert int(bt[0, 17:].abs().sum()) == 0 and int(bt[3:].abs().sum()) == 0
    assert c["k_cache"].shape[0] == 21
    # the ramp continues through the tail of the last block
    k, _ = gather_kv(c["k_cache"].double(), c["v_cache"].double(), bt[0], 272)
    assert float(k[271, 0, 0]) == 68.0 and float(k[255, 0, 0]) == 63.75


# ---------------------------------------------------------------------------
# rejected
# ---------------------------------------------------------------------------

def _mid(L):
    return (L // BS) // 2


# name -> (applies(L, window), kernel(family, L, window) -> output)
def _masked(**kw):
    def run(family, L, window):
        c, q, k, v = _case(family, L)
        return _exact(q, k, v, _mask(L, k.shape[0], window, **kw), c["scale"])
    return run


def _dropped(which):
    def run(family, L, window):
        c, q, k, v = _case(family, L)
        blk = {"first": 0, "mid": _mid(L), "last": (L - 1) // BS}[which]
        return _exact(q, k, v, _mask(L, k.shape[0], window, drop_block=blk),
                      c["scale"])
    return run


def _swapped(which):
    def run(family, L, window):
        c, q, k, v = _case(family, L)
        a, b = {"ends": (0, (L - 1) // BS),
                "neighbours": (_mid(L), _mid(L) + 1)}[which]
        return _exact(q, _swap_blocks(k, a, b), _swap_blocks(v, a, b),
                      _mask(L, k.shape[0], window), c["scale"])
    return run


def _no_rescale(family, L, window):
    c, q, k, v = _case(family, L)
    return _emulate(q, k, v, _mask(L, k.shape[0], window), c["scale"],
                    rescale_o=False)


_always = lambda L, window: True            # noqa: E731
_windowed = lambda L, window: window > 0    # noqa: E731

MUTANTS = {
    "causal+1": (_always, _masked(causal_shift=1)),
    "causal-1": (_always, _masked(causal_shift=-1)),
    "window_edge+1": (_windowed, _masked(window_shift=1)),
    "window_edge-1": (_windowed, _masked(window_shift=-1)),
    "drop_first_block": (_always, _dropped("first")),
    "drop_mid_block": (_always, _dropped("mid")),
    "drop_last_block": (_always, _dropped("last")),
    "swap_end_blocks": (_always, _swapped("ends")),
    "swap_neighbour_blocks": (_always, _swapped("neighbours")),
    "no_rescale_of_o": (_always, _no_rescale),
}


@pytest.mark.parametrize(
    "mutant,L,window",
    [(m, L, w) for m in MUTANTS for L, w in SHAPES if MUTANTS[m][0](L, w)])
def test_rejects_mutant(mutant, L, window):
    kernel = MUTANTS[mutant][1]
    rejected = {}
    for family in FAMILIES:
        out, a = _oracle(family, L, window)
        rejected[family] = not accepts(kernel(family, L, window), out, a)
    assert any(rejected.values()), (mutant, L, window, rejected)


@pytest.mark.parametrize("L,window", SHAPES)
def test_edge_mutants_are_order_one_on_the_ramps(L, window):
    """The ramps were built so an edge off by one key is no marginal
    miss: at least 10x the bound on the rows it touches."""
    out, a = _oracle("ramp_up", L, window)
    for shift in (1, -1):
        got = MUTANTS[f"causal{shift:+d}"][1]("ramp_up", L, window)
        assert worst_ratio(got, out, a) > 10
    if window:
        out, a = _oracle("ramp_down", L, window)
        for shift in (1, -1):
            got = MUTANTS[f"window_edge{shift:+d}"][1]("ramp_down", L, window)
            assert worst_ratio(got, out, a) > 10
