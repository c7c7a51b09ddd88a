"""fp64 oracle, derived error bound and input families for the paged
attention tests (test_attention_paths_gpu.py on the GPU,
test_attention_oracle.py for the CPU self-check of this checker).

The oracle
----------
``oracle_prefill`` / ``oracle_decode`` compute paged attention in fp64 over
the very tensors the kernel receives (bf16 q, bf16 or e5m2 cache — both
convert to fp64 exactly), with the semantics of ``kubeai_amd/ops/ref.py``:
query position p attends keys ``j <= p``, with a window only keys in
``(p - window, p]``, and the softcap ``c * tanh(s / c)`` is applied to the
scaled score before masking. Besides ``out = softmax(s) @ V`` they return
``A = softmax(s) @ |V|``, the scale against which rounding of the weights
shows up in an output element.

The bound
---------
``|kernel - out| <= 2**-7 * A + 2**-8 * |out| + 1e-6``, elementwise.

The kernels compute ``o = sum_j p_j v_j / l`` with ``l = sum_j p_j``:

* the MFMA kernels round each ``p_j`` to bf16 before the PV product:
  a relative error of at most 2**-9 per weight (8 significand bits, round
  to nearest), so the numerator moves by at most ``2**-9 * sum p_j |v_j|``,
  which after the division is ``2**-9 * A``;
* ``l`` is summed in fp32 from the *unrounded* ``p_j``, so it is not the
  sum of the weights that actually multiplied V. The mismatch is again at
  most 2**-9 relative, and ``|o| <= A``: another ``2**-9 * A``;
* the result is rounded to bf16: ``2**-9 * |out|``;
* fp32 score accumulation, ``__expf`` and the fp32 PV accumulation err at
  the 1e-6 .. 1e-5 relative level, orders below the terms above (the
  absolute 1e-6 keeps the comparison meaningful where ``out`` and ``A``
  both vanish).

That is ``2**-8 * A + 2**-9 * |out|``; the bound is that, doubled. A stale
running maximum (the defer-max shortcut keeps a maximum up to 8 below the
true one) changes no term: numerator and ``l`` carry the same factor.
The bound is derived, not measured — a kernel that exceeds it has an
approximation this derivation does not know about.

Input families
--------------
Coordinate 0 of q and k is reserved for structure, the other coordinates
carry ``0.5 * randn`` noise (score noise of std ~0.25), V is ``randn``:

* ``randn``     — q, k, v all N(0, 1): the generic case.
* ``ramp_up``   — ``s[i, j] ~ rate_i * j`` with ``rate_i = (i % 8) / 8``
  (``k[j, 0] = j / 4``; bf16/e5m2 rounding stair-steps it for large j, the
  oracle sees the same rounded values). Across a 64-key tile the row
  maximum grows by 0, 8, .. 56 depending on the row, so neighbouring rows
  need different rescale factors, and the mass sits on the LAST allowed
  key: a causal bound off by one key is an O(1) error.
* ``ramp_down`` — the same with negative rates: mass on the FIRST allowed
  key, which pins the lower window edge ``p - window + 1``; in split
  decode the first split dominates and later ones underflow in the merge.
* ``needle``    — (decode) key ``p`` of the sequence scores ~12 above the
  rest, ``out ~ V[p]``: a token lost at any block, wave or split boundary
  is an O(1) error.

K and V are generated for whole cache blocks, so the slots of the last
block beyond ``seq_len`` continue the pattern (under ``ramp_up`` they would
dominate if a kernel read them). Block tables are ``randperm`` physical
blocks; block 0 is reserved as the padding block and entries beyond a
sequence's need point at it.
"""
from __future__ import annotations

import math

import torch

BS = 16  # cache block size (tokens)

FAMILIES = ("randn", "ramp_up", "ramp_down")


# ---------------------------------------------------------------------------
# oracle
# ---------------------------------------------------------------------------

def _f64(t: torch.Tensor) -> torch.Tensor:
    return t.float().double()  # bf16 and e5m2 both widen exactly


def gather_kv(k_cache, v_cache, table, n_tok):
    """Logical [n_tok, n_kv, hd] K, V of one sequence (caches already
    widened: e5m2 tensors are converted whole, not indexed)."""
    n_blocks = (n_tok + BS - 1) // BS
    blocks = table[:n_blocks].long()
    k = k_cache[blocks].transpose(1, 2).reshape(
        -1, k_cache.shape[1], k_cache.shape[3])
    v = v_cache[blocks].transpose(1, 2).reshape(
        -1, v_cache.shape[1], v_cache.shape[3])
    return k[:n_tok], v[:n_tok]


def scores(qf, k, scale, softcap=0.0):
    """[n_q, rows, keys] fp64 scaled (and capped) scores, unmasked."""
    g = qf.shape[1] // k.shape[1]
    s = torch.einsum("qhd,lhd->hql", qf, k.repeat_interleave(g, dim=1)) * scale
    if softcap > 0:
        s = softcap * torch.tanh(s / softcap)
    return s


def visible(qpos, n_keys, window=0):
    """[rows, keys] bool: key j visible to the query at position qpos."""
    kpos = torch.arange(n_keys, device=qpos.device).unsqueeze(0)
    qp = qpos.unsqueeze(1)
    vis = kpos <= qp
    if window > 0:
        vis &= kpos > qp - window
    return vis


def _attend(qf, k, v, qpos, scale, window, softcap):
    s = scores(qf, k, scale, softcap)
    s = s.masked_fill(~visible(qpos, k.shape[0], window).unsqueeze(0),
                      float("-inf"))
    p = torch.softmax(s, dim=-1)
    vf = v.repeat_interleave(qf.shape[1] // v.shape[1], dim=1)
    out = torch.einsum("hql,lhd->qhd", p, vf)
    a = torch.einsum("hql,lhd->qhd", p, vf.abs())
    return out, a


def oracle_prefill(q, k_cache, v_cache, block_tables, query_start_loc,
                   seq_lens, scale, window=0, softcap=0.0):
    """fp64 (out, A), each [Tq, n_q, hd]."""
    out = torch.zeros(q.shape, dtype=torch.float64, device=q.device)
    a = torch.zeros_like(out)
    qsl = query_start_loc.tolist()
    kc, vc = _f64(k_cache), _f64(v_cache)
    for b, L in enumerate(seq_lens.tolist()):
        s0, s1 = qsl[b], qsl[b + 1]
        k, v = gather_kv(kc, vc, block_tables[b], L)
        qpos = torch.arange(L - (s1 - s0), L, device=q.device)
        out[s0:s1], a[s0:s1] = _attend(_f64(q[s0:s1]), k, v, qpos, scale,
                                       window, softcap)
    return out, a


def oracle_decode(q, k_cache, v_cache, block_tables, seq_lens, scale,
                  window=0, softcap=0.0):
    """fp64 (out, A), each [B, n_q, hd]: the query of sequence b sits at
    position seq_lens[b] - 1."""
    B = q.shape[0]
    qsl = torch.arange(B + 1, dtype=torch.int32)
    return oracle_prefill(q, k_cache, v_cache, block_tables, qsl, seq_lens,
                          scale, window, softcap)


# ---------------------------------------------------------------------------
# the check
# ---------------------------------------------------------------------------

def error_bound(out, a):
    return 2.0 ** -7 * a + 2.0 ** -8 * out.abs() + 1e-6


def worst_ratio(got, out, a) -> float:
    """max over elements of |got - out| / bound; inf for a non-finite
    kernel output."""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - out).abs() / error_bound(out, a)).max())


def accepts(got, out, a) -> bool:
    return worst_ratio(got, out, a) <= 1.0


def assert_within_bound(got, out, a, label=""):
    r = worst_ratio(got, out, a)
    print(f"ATTN_RATIO {label} {r:.3f}")
    if r > 1.0:
        err = (got.double() - out).abs()
        bad = err > error_bound(out, a)
        idx = bad.nonzero()[0].tolist()
        rows = bad.flatten(1).any(1).nonzero().flatten().tolist()
        raise AssertionError(
            f"{label}: worst err/bound {r:.2f}; {int(bad.sum())} of "
            f"{bad.numel()} elements over the bound, first at {idx} "
            f"(got {float(got[tuple(idx)]):.5f}, want "
            f"{float(out[tuple(idx)]):.5f}); rows {rows[:16]}")
    return r


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

def _rate(rows, heads):
    """[rows, heads] ramp rate (row + head) % 8 / 8."""
    r = torch.arange(rows).unsqueeze(1) + torch.arange(heads).unsqueeze(0)
    return (r % 8).float() / 8.0


def make_case(family, q_lens, ctx_lens, n_q, n_kv, hd=128,
              cache_dtype=torch.bfloat16, device="cpu", seed=0,
              table_pad=1, pad_rows=0, needle_pos=None):
    """One paged-attention problem. Decode cases pass ``q_lens`` of all 1.

    table_pad widens the block table to table_pad x the needed width (extra
    entries 0); pad_rows appends that many seq_len = 1 rows whose table is
    all block 0 (the shape of a graph-padded decode batch). needle_pos[b]
    is the key position of the needle for family "needle".

    Returns a dict with q [Tq, n_q, hd] bf16, k_cache / v_cache
    [nb, n_kv, 16, hd], block_tables int32 [B, width], query_start_loc
    int32 [B + 1], seq_lens int32 [B], scale.
    """
    gen = torch.Generator().manual_seed(seed)

    def randn(*shape):
        return torch.randn(*shape, generator=gen)

    scale = 1.0 / math.sqrt(hd)
    B = len(q_lens)
    lens = [a + c for a, c in zip(q_lens, ctx_lens)]
    n_blk = [(L + BS - 1) // BS for L in lens]
    total = sum(n_blk)
    Tq = sum(q_lens)
    structured = family != "randn"
    amp = 0.5 if structured else 1.0

    q = amp * randn(Tq, n_q, hd)
    if family in ("ramp_up", "ramp_down"):
        sign = 1.0 if family == "ramp_up" else -1.0
        q[:, :, 0] = sign * _rate(Tq, n_q) * 4.0 / scale
    elif family == "needle":
        q[:, :, 0] = 12.0 / (scale * 8.0)
    elif family != "randn":
        raise ValueError(family)

    # physical blocks: 0 is the padding block, the rest shuffled
    perm = (torch.randperm(total, generator=gen) + 1).to(torch.int32)
    k_cache = randn(total + 1, n_kv, BS, hd)
    v_cache = randn(total + 1, n_kv, BS, hd)
    width = max(n_blk) * table_pad
    bt = torch.zeros(B + pad_rows, width, dtype=torch.int32)
    at = 0
    for b in range(B):
        nbk = n_blk[b]
        blocks = perm[at:at + nbk]
        at += nbk
        bt[b, :nbk] = blocks
        k = amp * randn(nbk * BS, n_kv, hd)
        if family in ("ramp_up", "ramp_down"):
            k[:, :, 0] = (torch.arange(nbk * BS).float() / 4.0).unsqueeze(1)
        elif family == "needle":
            k[:, :, 0] = 0.0
            k[needle_pos[b], :, 0] = 8.0
        k_cache[blocks.long()] = k.view(nbk, BS, n_kv, hd).transpose(1, 2)
    if pad_rows:
        lens = lens + [1] * pad_rows
        q_lens = list(q_lens) + [1] * pad_rows
        q = torch.cat([q, randn(pad_rows, n_q, hd)])
    qsl = torch.tensor([0] + list(torch.tensor(q_lens).cumsum(0)),
                       dtype=torch.int32)
    return dict(
        q=q.to(torch.bfloat16).to(device),
        k_cache=k_cache.to(cache_dtype).to(device),
        v_cache=v_cache.to(cache_dtype).to(device),
        block_tables=bt.to(device),
        query_start_loc=qsl.to(device),
        seq_lens=torch.tensor(lens, dtype=torch.int32).to(device),
        scale=scale,
    )
