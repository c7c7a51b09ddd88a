"""ops.lora_apply on the GPU (csrc/lora_batched.hip) against an fp64 reference
over the very bf16 tensors the kernels get (tests/lora_util.py), and the
graph-captured decode step with adapters loaded."""
import pytest
import torch

from kubeai_amd import ops
from kubeai_amd.engine import EngineConfig, LLMEngine, SamplingParams
from kubeai_amd.engine.lora import LoraTable
from kubeai_amd.engine.scheduler import Request, ScheduledSeq, SchedulerOutput
from lora_util import reference

pytestmark = pytest.mark.gpu

# slot -> rank; slot 5 keeps R = 0 and slot 6 has an adapter no row names
RANKS = {1: 8, 2: 16, 3: 48, 4: 64, 6: 16}
MIXED = [1, 0, 2, 5, 3, 4, 0, 4, 2]


def _case(T, K, N, pattern, draw, scales):
    """(y0, x, slots, table) on the GPU; x is a row-strided view.
    draw(kind, shape) makes the bf16 data, scales[slot % 4] the slots' scales."""
    table = LoraTable(K, N, "cuda")
    for slot, R in RANKS.items():
        table.set_row(slot, draw("A", (R, K)).cuda(), draw("B", (N, R)).cuda(),
                      scales[slot % 4])
    x = draw("x", (T, K + 8)).cuda()[:, :K]
    y0 = draw("y", (T, N)).cuda()
    cycle = MIXED if pattern == "mixed" else [4]
    slots = torch.tensor((cycle * T)[:T], dtype=torch.int32, device="cuda")
    return y0, x, slots, table


@pytest.mark.parametrize("N", [48, 272])
@pytest.mark.parametrize("K", [64, 1032])
@pytest.mark.parametrize("T,pattern", [(1, "mixed"), (17, "mixed"),
                                       (64, "mixed"), (64, "one")])
def test_exact_map(T, pattern, K, N):
    """Small integers and power-of-two scales: every product, sum and
    rounding is exact, so the output is the reference bit for bit and a wrong
    k-slot, rank mask, row list or column tile is a wrong integer."""
    g = torch.Generator().manual_seed(K + N + T)

    def draw(kind, shape):
        # all in {-1, 0, 1}, x and B thinned to 1/4: |A x| stays below 256
        # and y below 256 units of the scale, so both are exact in bf16
        v = torch.randint(-1, 2, shape, generator=g)
        if kind in "xB":
            v = v * (torch.rand(shape, generator=g) < 0.25)
        return v.bfloat16()

    y0, x, slots, table = _case(T, K, N, pattern, draw, [1.0, 0.5, 0.25, 0.125])
    ref, _ = reference(y0, x, slots, table.rows)
    for s, (A, _, _) in ((s, r) for s, r in enumerate(table.rows) if r):
        assert (x.double() @ A.double().T).abs().max() <= 256  # the data's claim
    assert torch.equal(ref.bfloat16().double(), ref)
    y = y0.clone()
    ops.lora_apply(y, x, slots, table)
    assert torch.equal(y.double().cpu(), ref)
    idle = ((slots == 0) | (slots == 5)).cpu()
    assert torch.equal(y.cpu()[idle], y0.cpu()[idle])
    assert pattern == "one" or T == 1 or (idle.any() and not idle.all())


@pytest.mark.parametrize("T,K,N", [(17, 1032, 272), (64, 4096, 128)])
def test_random_within_bound(T, K, N):
    g = torch.Generator().manual_seed(T)
    draw = lambda kind, shape: torch.randn(shape, generator=g).bfloat16()
    y0, x, slots, table = _case(T, K, N, "mixed", draw, [0.125, 0.03, 0.25, 0.07])
    ref, bound = reference(y0, x, slots, table.rows)
    y = y0.clone()
    ops.lora_apply(y, x, slots, table)
    ratio = ((y.double().cpu() - ref).abs() / bound).max().item()
    print(f"lora_apply T={T} K={K} N={N}: worst err / bound = {ratio:.3f}")
    assert ratio <= 1.0


def test_graph_replay():
    """A captured apply reads slots, table and x at replay: after all three
    are rewritten in place it gives the eager result of the new contents."""
    g = torch.Generator().manual_seed(5)
    draw = lambda kind, shape: torch.randn(shape, generator=g).bfloat16()
    T, K, N = 17, 1032, 272
    y0, x, slots, table = _case(T, K, N, "mixed", draw, [0.125, 0.03, 0.25, 0.07])
    x = x.contiguous()
    vpart = ops.lora_vpart("cuda", T)
    y = y0.clone()
    ops.lora_apply(y, x, slots, table, vpart)  # loads the code objects
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y.copy_(y0)
        ops.lora_apply(y, x, slots, table, vpart)
    slots.copy_(slots.flip(0))
    table.set_row(2, draw("A", (64, K)).cuda(), draw("B", (N, 64)).cuda(), 0.01)
    x.copy_(draw("x", (T, K)).cuda())
    want = y0.clone()
    ops.lora_apply(want, x, slots, table, vpart)
    for _ in range(3):
        graph.replay()
        assert torch.equal(y, want)
    assert not torch.equal(want, y0)


@pytest.mark.parametrize("bad", ["T", "K", "rank", "slots"])
def test_host_errors(bad):
    T, K = (65 if bad == "T" else 4), (60 if bad == "K" else 64)
    table = LoraTable(K, 48, "cuda")
    x = torch.zeros(T, K, dtype=torch.bfloat16, device="cuda")
    y = torch.zeros(T, 48, dtype=torch.bfloat16, device="cuda")
    slots = torch.zeros(T, dtype=torch.int64 if bad == "slots" else torch.int32,
                        device="cuda")
    if bad == "rank":
        A = torch.zeros(12, K, dtype=torch.bfloat16, device="cuda")
        B = torch.zeros(48, 12, dtype=torch.bfloat16, device="cuda")
        with pytest.raises(RuntimeError):
            table.set_row(1, A, B, 1.0)
        table.host[1, 2] = table.dev[1, 2] = 12  # past set_row's own check
    with pytest.raises(RuntimeError):
        ops.lora_apply(y, x, slots, table)


def test_engine_decode_graph():
    """A pure-decode step with adapters loaded runs through a captured graph
    of its own; base rows keep their bits, adapter rows move, and an unloaded
    adapter's slot adds nothing at the next replay."""
    eng = LLMEngine(EngineConfig(model="llama-tiny", device="cuda",
                                 max_model_len=512, num_gpu_blocks=256, seed=0))
    runner = eng.runner
    runner.load_lora(1, None)
    runner.load_lora(2, None)

    def step(lora_ids):
        seqs = []
        for i, lid in enumerate(lora_ids):
            req = Request(list(range(20, 25)), SamplingParams(max_tokens=4),
                          request_id=f"r{i}", lora_id=lid)
            req.block_table = [i + 1]
            seqs.append(ScheduledSeq(req, 4, 1))
        return SchedulerOutput(decode=seqs, prefill=[], preempted=[])

    runner.execute(step([1, 2, 0]), 0)
    assert ("lora", 8) in runner._graphs
    @torch.inference_mode()
    def logits(lora_ids):
        return runner._execute_graph(step(lora_ids), lora=True).float().clone()

    mixed, base = logits([1, 2, 0]), logits([0, 0, 0])
    assert torch.equal(mixed[2], base[2])
    for row in (0, 1):
        diff = (mixed[row] - base[row]).abs().max().item()
        assert diff > 0.05, f"adapter row {row} did not move (max diff {diff})"
    lm = runner.lora_manager
    slot = lm.slot_of(2)
    runner.unload_lora(2)
    lm.slots[2] = slot  # row 1 still names the slot: its rows are R = 0 now
    after = logits([1, 2, 0])
    del lm.slots[2]
    assert torch.equal(after[1], base[1])
    assert torch.equal(after[0], mixed[0])
