"""LLMEngine — the per-GPU serving engine facade.

add_request() / step() / abort(); one step = schedule -> forward -> commit.
This is the in-house replacement for the vLLM container the reference
launches per Model pod.
"""
from __future__ import annotations

import dataclasses
import time
from typing import Optional

import torch

from kubeai_amd.models.config import ModelArchConfig, PRESETS

from .kvcache import BlockManager
from .runner import ModelRunner, self_feed_ok
from .scheduler import Request, SamplingParams, Scheduler


class RequestError(ValueError):
    """Client error in a request body -> HTTP 400."""


@dataclasses.dataclass
class EngineConfig:
    model: str = "llama-tiny"  # preset name or HF dir
    device: str = "auto"  # auto -> cuda if available else cpu
    dtype: str = "bfloat16"
    block_size: int = 16
    num_gpu_blocks: Optional[int] = None  # None -> profile from free HBM
    gpu_memory_utilization: float = 0.90
    max_num_seqs: int = 256
    max_num_batched_tokens: int = 8192
    max_model_len: int = 8192
    enable_prefix_caching: bool = True
    # "fp8"  => W8A8 dynamic (quant.py)
    # "int4" => W4A16 (quant_int4.py): AWQ-gemm checkpoints are served from
    #           their packed codes, float weights are quantized round-to-
    #           nearest (g=128); lm_head stays bf16; not with tensor parallelism
    # "mxfp4" => W4A8 (quant_mxfp4.py): OCP microscaling FP4 weights, quantized
    #           round-to-nearest; decode steps run on the scaled MFMA from the
    #           fp8 producers' rows; lm_head stays bf16; dense models only, not
    #           with tensor parallelism
    quantization: Optional[str] = None
    # "auto" = model dtype; "fp8_e5m2" halves KV bytes + doubles capacity
    kv_cache_dtype: str = "auto"
    enable_graphs: bool = True  # hipGraph capture for pure-decode steps
    prefill_interval: int = 1  # >1: batch prefills onto every Nth step
    seed: int = 0

    def resolve_arch(self) -> ModelArchConfig:
        if self.model in PRESETS:
            return PRESETS[self.model]
        return ModelArchConfig.from_hf_config(self.model)

    def resolve_device(self) -> str:
        if self.device != "auto":
            return self.device
        return "cuda" if torch.cuda.is_available() else "cpu"


@dataclasses.dataclass
class RequestOutput:
    request_id: str
    new_token_ids: list[int]
    finished: bool
    finish_reason: Optional[str]  # "stop" | "length" | "abort"
    num_prompt_tokens: int
    num_cached_tokens: int
    output_token_ids: list[int]
    logprob: Optional[float] = None  # logprob of new_token_ids[-1]
    # top alternatives for new_token_ids[-1]: [(token_id, logprob), ...]
    top_logprobs: Optional[list] = None


class LLMEngine:
    def __init__(self, cfg: EngineConfig, tp_group=None):
        self.cfg = cfg
        arch = cfg.resolve_arch()
        self.arch = arch
        device = cfg.resolve_device()
        self.runner = ModelRunner(
            arch,
            device=device,
            dtype=getattr(torch, cfg.dtype),
            block_size=cfg.block_size,
            num_gpu_blocks=cfg.num_gpu_blocks,
            gpu_memory_utilization=cfg.gpu_memory_utilization,
            seed=cfg.seed,
            tp_group=tp_group,
            max_model_len=cfg.max_model_len,
            enable_graphs=cfg.enable_graphs,
            quantization=cfg.quantization,
            model_path=cfg.model,
            kv_cache_dtype=cfg.kv_cache_dtype,
        )
        self.block_manager = BlockManager(self.runner.num_blocks, cfg.block_size)
        self.scheduler = Scheduler(
            self.block_manager,
            max_num_seqs=cfg.max_num_seqs,
            max_num_batched_tokens=cfg.max_num_batched_tokens,
            max_model_len=cfg.max_model_len,
            enable_prefix_caching=cfg.enable_prefix_caching,
            prefill_interval=cfg.prefill_interval,
        )
        self.step_count = 0

    # ------------------------------------------------------------------
    def add_request(
        self,
        prompt_token_ids: list[int],
        params: Optional[SamplingParams] = None,
        request_id: Optional[str] = None,
        lora_id: int = 0,
        images: Optional[list] = None,
    ) -> Request:
        if params is None:
            params = SamplingParams()
        if not params.ignore_eos and self.arch.eos_token_id not in params.stop_token_ids:
            params = dataclasses.replace(
                params,
                stop_token_ids=tuple(params.stop_token_ids)
                + (self.arch.eos_token_id,),
            )
        mm_spans: list[tuple[int, int, int]] = []
        if images:
            # expand each image-placeholder token to n_patches positions
            # (vLLM-style); the runner replaces those embedding rows with
            # the vision-tower output
            if self.arch.vision is None:
                raise RequestError(
                    f"model {self.cfg.model!r} does not accept image input"
                )
            img_id = self.arch.image_token_id
            n_patch = self.runner.vision.n_patches
            n_slots = sum(1 for t in prompt_token_ids if t == img_id)
            if n_slots != len(images):
                raise RequestError(
                    f"prompt has {n_slots} image slot(s) but request "
                    f"carries {len(images)} image(s)"
                )
            expanded: list[int] = []
            k = 0
            for t in prompt_token_ids:
                if t == img_id:
                    mm_spans.append((len(expanded), n_patch, k * n_patch))
                    expanded.extend([img_id] * n_patch)
                    k += 1
                else:
                    expanded.append(t)
            prompt_token_ids = expanded
            if len(prompt_token_ids) >= self.cfg.max_model_len:
                raise RequestError(
                    "multimodal prompt exceeds max_model_len "
                    "(image spans cannot be truncated)"
                )
        if len(prompt_token_ids) >= self.cfg.max_model_len:
            prompt_token_ids = prompt_token_ids[-(self.cfg.max_model_len - 1) :]
        req = Request(prompt_token_ids, params, request_id=request_id, lora_id=lora_id)
        if images:
            req.images = list(images)
            req.mm_spans = mm_spans
            # salt the prefix cache with image content: same token ids,
            # different pixels -> different KV
            req.cache_salt = hash(
                (lora_id,)
                + tuple(hash(im.numpy().tobytes()) for im in req.images)
            )
        self.scheduler.add_request(req)
        return req

    def abort_request(self, request_id: str) -> None:
        self.scheduler.abort(request_id)
        self.runner.release_request(request_id)

    def has_work(self) -> bool:
        return self.scheduler.has_work()

    # ------------------------------------------------------------------
    def _predict_run_ahead(self, out) -> bool:
        """Will the step after `out` be `out`'s decode batch again, whatever
        tokens `out` samples (a stop token aside)? If so, grow the block
        tables for it and tell the runner to enqueue that step's replay
        before it waits for this step's tokens. The host then does this
        step's bookkeeping while the device runs the next one; the next
        step() adopts the replay if the scheduler decides as predicted, and
        lets it finish unused if not (runner.runahead_stats)."""
        runner, sched = self.runner, self.scheduler
        if (
            not runner.self_feed
            or out.prefill
            or out.preempted
            or not out.decode
            or len(out.decode) != len(sched.running)
            or sched._aborted
        ):
            return False
        lm = getattr(runner, "lora_manager", None)
        if lm is not None and lm.active:
            return False
        reqs = [ss.req for ss in out.decode]
        for r in reqs:
            if not self_feed_ok(r.params):
                return False
            # ends by length in this step: the batch changes
            if (
                r.num_generated + 1 >= r.params.max_tokens
                or len(r.tokens) + 1 >= sched.max_model_len
            ):
                return False
        next_defers = (
            sched.prefill_interval > 1
            and (sched._step_idx + 1) % sched.prefill_interval != 0
        )
        if sched.waiting and not next_defers:
            return False  # the next step admits a prefill
        # The replay ahead writes the cache row of position num_computed + 1
        # of each request and reads the rows before it: it touches only
        # blocks the batch owns. A request at a block boundary gets the next
        # block now, the one the scheduler would append one step later; if
        # the pool cannot give it without preempting, nothing runs ahead.
        # ModelRunner._run_ahead asserts this before it enqueues.
        bs = self.cfg.block_size
        grow = [r for r in reqs if len(r.block_table) * bs < r.num_computed + 2]
        if len(grow) > self.block_manager.num_free_blocks:
            return False
        for r in grow:
            self.block_manager.append_block(r.block_table)
        return True

    def step(self) -> list[RequestOutput]:
        if self.scheduler._aborted:
            # an abort frees blocks the replay ahead may still write to
            self.runner.wait_inflight()
        out = self.scheduler.schedule()
        results: list[RequestOutput] = []
        for req in out.rejected:
            results.append(
                RequestOutput(
                    request_id=req.request_id,
                    new_token_ids=[],
                    finished=True,
                    finish_reason="abort",
                    num_prompt_tokens=req.num_prompt_tokens,
                    num_cached_tokens=0,
                    output_token_ids=[],
                )
            )
        if out.is_empty:
            self.runner.drop_inflight()
            return results
        sampled = self.runner.execute(
            out, self.step_count, run_ahead=self._predict_run_ahead(out)
        )
        self.step_count += 1
        now = time.monotonic()
        # A request that ends here on a stop token is still a row of the
        # replay enqueued ahead, which writes one more cache row into the
        # request's last block: the blocks go back only once it has run.
        held: Optional[list] = [] if self.runner._inflight is not None else None
        finished = self.scheduler.finish_step(out, sampled, now, defer_free=held)
        if held:
            self.runner.wait_inflight()
            for table in held:
                self.block_manager.free(table)
            if not self.scheduler.running:
                self.runner.drop_inflight()  # no step will come for it
        finished_ids = {r.request_id for r in finished}
        for rid in finished_ids:
            self.runner.release_request(rid)
        for ss in out.all_seqs:
            req = ss.req
            if not ss.samples:
                continue
            tok = sampled[req.request_id]
            results.append(
                RequestOutput(
                    request_id=req.request_id,
                    new_token_ids=[tok],
                    finished=req.request_id in finished_ids,
                    finish_reason=req.status.value if req.status.finished else None,
                    num_prompt_tokens=req.num_prompt_tokens,
                    num_cached_tokens=req.num_cached_prompt_tokens,
                    output_token_ids=req.output_token_ids,
                    logprob=getattr(self.runner, "last_logprobs", {}).get(
                        req.request_id
                    ),
                    top_logprobs=getattr(self.runner, "last_top_logprobs", {}).get(
                        req.request_id
                    ),
                )
            )
        return results

    # ------------------------------------------------------------------
    def embed(self, tok_lists: list[list[int]]) -> list[list[float]]:
        """Mean-pooled, L2-normalised final hidden states (TextEmbedding
        feature; reference analog: the Infinity engine).

        Sequences are packed many-per-forward (token-budget bounded), the
        same packed-prefill shape the generation path uses — batched
        embedding throughput instead of one forward per input.

        MUST run on the stepping thread (the server routes embed jobs
        through its submit loop): it shares the BlockManager and KV
        tensors with in-flight generations.
        """
        from .scheduler import ScheduledSeq, SchedulerOutput

        out: list[Optional[list[float]]] = [None] * len(tok_lists)
        budget = self.cfg.max_num_batched_tokens
        i = 0
        while i < len(tok_lists):
            batch: list[tuple[int, Request, list[int]]] = []
            total = 0
            while i < len(tok_lists):
                toks = list(tok_lists[i][: self.cfg.max_model_len - 1])
                if batch and total + len(toks) > budget:
                    break
                table, _ = self.block_manager.allocate(toks, salt=-1, max_cached=0)
                req = Request(toks, SamplingParams(max_tokens=1))
                req.block_table = table
                batch.append((i, req, toks))
                total += len(toks)
                i += 1
            so = SchedulerOutput(
                decode=[],
                prefill=[ScheduledSeq(r, 0, len(t)) for _, r, t in batch],
                preempted=[],
            )
            fb = self.runner.build_batch(so)
            hidden = self.runner.model(fb)
            ofs = 0
            for idx, req, toks in batch:
                # rows are packed prefill-order; bucket padding sits past
                # the real tokens
                vec = hidden[ofs : ofs + len(toks)].float().mean(dim=0)
                vec = vec / vec.norm().clamp_min(1e-12)
                out[idx] = vec.cpu().tolist()
                ofs += len(toks)
                self.block_manager.free(req.block_table)
        return out

    # ------------------------------------------------------------------
    # LoRA adapter lifecycle (weights managed by the runner's LoRA manager)
    def load_lora(self, lora_id: int, path: Optional[str]) -> None:
        self.runner.load_lora(lora_id, path)

    def unload_lora(self, lora_id: int) -> None:
        self.runner.unload_lora(lora_id)

    # ------------------------------------------------------------------
    # metrics for /metrics + the autoscaler
    def stats(self) -> dict:
        return {
            "num_running": self.scheduler.num_running,
            "num_waiting": self.scheduler.num_waiting,
            "kv_usage": self.block_manager.usage(),
            "prefix_cache_hit_rate": self.block_manager.hit_rate(),
            "step_count": self.step_count,
            # decode run-ahead: replays enqueued before the step's tokens
            # were read, and what became of them at the next step
            "runahead_enqueued": self.runner.runahead_stats["enqueued"],
            "runahead_adopted": self.runner.runahead_stats["adopted"],
            "runahead_discarded": self.runner.runahead_stats["discarded"],
        }
