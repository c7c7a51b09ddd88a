"""Shared cases for the decode run-ahead tests (CPU and GPU files)."""
import struct

import numpy as np
import torch

BS = 16      # block size of every case
BT_MAX = 8   # table width of the decode_advance cases

ADVANCE_CASES = [(1, 8), (5, 8), (1, 64), (5, 64), (40, 64)]  # (B, b_pad)


def advance_case(B: int, b_pad: int, device="cpu"):
    """Inputs of one decode_advance call and, computed here with plain
    Python, what it must leave behind. Row kinds, cycled over the rows:
      stay   position 3 -> 4, inside the first block
      cross  position 16k+15 -> 16k+16, the first cell of the next block
      last   crosses into the table's last entry (BT_MAX - 1)
      mid    somewhere inside a middle block
      frozen at a block boundary without a block for the next position
    B == 1 takes `cross`. Pad rows hold the padded upload's values."""
    rng = np.random.RandomState(100 * B + b_pad)
    kinds = ["cross"] if B == 1 else ["stay", "cross", "last", "mid", "frozen"]
    ids = np.zeros(b_pad, np.int32)
    pos = np.zeros(b_pad, np.int32)
    slots = np.full(b_pad, -1, np.int64)
    lens = np.ones(b_pad, np.int32)
    tables = np.zeros((b_pad, BT_MAX), np.int32)
    nb = np.zeros(b_pad, np.int32)
    tokens = rng.randint(0, 128256, size=b_pad).astype(np.int64)
    live = np.array([B], np.int32)
    exp = None
    want = {}
    for b in range(B):
        kind = kinds[b % len(kinds)]
        k = (b // len(kinds)) % (BT_MAX - 2)
        if kind == "stay":
            p, n = 3, 1
        elif kind == "cross":
            p, n = BS * k + BS - 1, k + 2
        elif kind == "last":
            p, n = BS * (BT_MAX - 1) - 1, BT_MAX
        elif kind == "mid":
            p, n = BS * (k + 1) + 5, k + 2
        else:
            p, n = BS * (k + 1) - 1, k + 1
        row = rng.permutation(1000)[:n].astype(np.int32) + 1
        tables[b, :n] = row
        nb[b] = n
        ids[b] = rng.randint(0, 128256)
        pos[b] = p
        lens[b] = p + 1
        slots[b] = int(row[p // BS]) * BS + p % BS
        if kind == "frozen":
            want[b] = (ids[b], p, slots[b], p + 1)
        else:
            q = p + 1
            want[b] = (tokens[b], q, int(row[q // BS]) * BS + q % BS, q + 1)
    exp = [ids.copy(), pos.copy(), slots.copy(), lens.copy()]
    for b, (i, p, s, n) in want.items():
        exp[0][b], exp[1][b], exp[2][b], exp[3][b] = i, p, s, n
    t = lambda a: torch.from_numpy(a.copy()).to(device)
    args = [t(ids), t(pos), t(slots), t(lens), t(tables), t(nb), t(live),
            t(tokens)]
    return args, [torch.from_numpy(e) for e in exp]


def bits(x):
    """A float's bit pattern (None stays None): equality bit for bit."""
    return None if x is None else struct.pack("<d", x)


REQUESTS = [  # (id, prompt length, max_tokens)
    ("r0", 21, 3), ("r1", 40, 4), ("r2", 35, 9), ("r3", 50, 17),
    # 30 + 17 tokens: the block boundary at 32 lies inside the run
    ("r4", 30, 17), ("r5", 26, 32),
]
# arrive before the engine's 8th step (prefills are admitted on every 4th) and
# before its 10th (not admitted until the 12th)
ARRIVALS = {8: ("a0", 23, 5), 10: ("a1", 44, 6)}


def run_traffic(device, stop=None, odd=None, num_gpu_blocks=256):
    """The run-ahead tests' seeded traffic through one engine. stop: (request
    id, token) gives that request ignore_eos=False and the stop token. odd:
    SamplingParams fields for r2 (a request the graph cannot sample).
    Returns (per-step outputs, free blocks at the end, stats, engine); stats
    is eng.stats() plus enqueued_by_step."""
    from kubeai_amd.engine import EngineConfig, LLMEngine, SamplingParams

    eng = LLMEngine(EngineConfig(
        model="llama-tiny", device=device, num_gpu_blocks=num_gpu_blocks,
        max_model_len=512, prefill_interval=4, seed=0,
    ))

    def add(rid, n_prompt, max_tokens):
        kw = dict(max_tokens=max_tokens, ignore_eos=True)
        if stop is not None and stop[0] == rid:
            kw.update(ignore_eos=False, stop_token_ids=(stop[1],))
        if odd is not None and rid == "r2":
            kw.update(odd)
        base = 7 + 97 * (int(rid[1:]) + (10 if rid[0] == "a" else 0))
        prompt = [(base + 13 * i) % 1000 + 3 for i in range(n_prompt)]
        eng.add_request(prompt, SamplingParams(**kw), request_id=rid)

    for r in REQUESTS:
        add(*r)
    steps, enqueued = [], []  # enqueued: replays ahead so far, after each step
    call = 0
    while eng.has_work() or call < max(ARRIVALS):
        call += 1
        assert call < 200
        if call in ARRIVALS:
            add(*ARRIVALS[call])
        steps.append([
            (o.request_id, tuple(o.new_token_ids), bits(o.logprob),
             o.finished, o.finish_reason, tuple(o.output_token_ids),
             o.num_prompt_tokens, o.num_cached_tokens)
            for o in eng.step()
        ])
        enqueued.append(eng.runner.runahead_stats["enqueued"])
    stats = dict(eng.stats(), enqueued_by_step=enqueued)
    return steps, eng.block_manager.num_free_blocks, stats, eng


def pick_stop(steps, rid="r5", at=6):
    """The `at`-th token that request `rid` generated in a finished run, if it
    did not generate it before: a stop token known to be emitted."""
    gen = [o for s in steps for o in s if o[0] == rid and o[3]][0][5]
    for i in range(at, len(gen) - 1):
        if gen[i] not in gen[:i]:
            return rid, gen[i]
    raise AssertionError(f"no usable stop token in {gen}")
