"""The batched multi-LoRA path off the GPU: adapter slots and table rows,
ForwardBatch.lora_slots, and the torch reference of ops.lora_apply."""
import torch

from kubeai_amd import ops
from kubeai_amd.engine import EngineConfig, LLMEngine, SamplingParams
from kubeai_amd.engine.scheduler import Request, ScheduledSeq, SchedulerOutput
from lora_util import reference


def _engine():
    return LLMEngine(EngineConfig(model="llama-tiny", device="cpu",
                                  num_gpu_blocks=64, max_model_len=256, seed=0))


def test_slots_and_table_rows():
    eng = _engine()
    eng.load_lora(5, None)
    eng.load_lora(9, None)
    lm = eng.runner.lora_manager
    assert (lm.slot_of(5), lm.slot_of(9), lm.slot_of(7)) == (1, 2, None)
    table = lm.tables["down"][1]
    A, B, _ = lm.adapters[5]["down"][1]
    assert table.host[1].tolist()[:3] == [A.data_ptr(), B.data_ptr(), 16]
    assert torch.equal(table.dev, table.host)
    eng.unload_lora(5)
    assert lm.slot_of(5) is None
    for tables in lm.tables.values():
        for t in tables:
            assert not t.dev[1].any() and not t.host[1].any() and t.rows[1] is None
            assert t.dev[2, 2] == 16  # adapter 9 stays where it is
    eng.load_lora(11, None)
    assert (lm.slot_of(11), lm.slot_of(9)) == (1, 2)  # the freed slot is reused
    assert lm.batched(8, True) and not lm.batched(65, True)
    assert not lm.batched(8, False)


def test_build_batch_lora_slots():
    eng = _engine()
    eng.load_lora(9, None)
    eng.load_lora(11, None)

    def seq(lora_id, start, length):
        req = Request(list(range(10, 18)), SamplingParams(max_tokens=1),
                      lora_id=lora_id)
        req.block_table = [1]
        return ScheduledSeq(req, start, length)

    # two decode rows, a 5-token prefill chunk of an adapter that is not
    # loaded and one of a loaded one: 9 rows, padded to 16
    out = SchedulerOutput(
        decode=[seq(11, 7, 1), seq(0, 7, 1)],
        prefill=[seq(4, 0, 5), seq(9, 0, 2)], preempted=[],
    )
    fb = eng.runner.build_batch(out)
    assert fb.lora_slots.dtype == torch.int32
    assert fb.lora_slots.tolist() == [2, 0] + [0] * 5 + [1] * 2 + [0] * 7
    assert fb.lora_ids.tolist() == [11, 0] + [4] * 5 + [9] * 2 + [0] * 7


def test_cpu_lora_apply_matches_adapter_loop():
    """ops.lora_apply's reference against LoRAManager.apply's per-adapter
    loop within the bound of the GPU test (tests/lora_util.py), on small
    integers with the synthetic adapters' power-of-two scale: every rounding
    of either path is then exact, so nothing but a different map can part
    them. On random data the two differ by up to 1.77 times that bound while
    each is within it of the fp64 reference (0.89 at most): the bound is one
    bf16 rounding of the output and one of v, and the loop rounds the output,
    v and B v on its own. Random data is therefore held against the fp64
    reference."""
    eng = _engine()
    eng.load_lora(9, None)
    eng.load_lora(11, None)
    lm = eng.runner.lora_manager
    table = lm.tables["gate_up"][0]
    g = torch.Generator().manual_seed(3)
    T = 19
    ids = torch.tensor([9, 0, 11, 11, 4] * 4, dtype=torch.int32)[:T]
    slots = torch.tensor([lm.slot_of(int(i)) or 0 for i in ids], dtype=torch.int32)
    for lid in (9, 11):  # integer weights in the manager and in the table
        A, B, scale = lm.adapters[lid]["gate_up"][0]
        A.copy_(torch.randint(-1, 2, A.shape, generator=g))
        B.copy_(torch.randint(-1, 2, B.shape, generator=g))
        assert table.rows[lm.slot_of(lid)][0] is A and scale == 0.125
    x = torch.randint(-1, 2, (T, table.K), generator=g).bfloat16()
    y0 = torch.randint(-4, 5, (T, table.N), generator=g).bfloat16()
    old, new = y0.clone(), y0.clone()
    lm.apply(0, "gate_up", x, old, ids)
    ops.lora_apply(new, x, slots, table)
    ref, bound = reference(y0, x, slots, table.rows)
    assert torch.equal(ref.bfloat16().double(), ref)  # the data's claim
    assert ((new.double() - old.double()).abs() <= bound).all()
    base = slots == 0
    assert torch.equal(new[base], y0[base]) and not torch.equal(new[~base], y0[~base])

    x = torch.randn(T, table.K, generator=g).bfloat16()
    y0 = torch.randn(T, table.N, generator=g).bfloat16()
    new = y0.clone()
    ops.lora_apply(new, x, slots, table)
    ref, bound = reference(y0, x, slots, table.rows)
    assert ((new.double() - ref).abs() <= bound).all()
