"""Continuous-batching generation engine for the VLM decoder (paged KV cache, TP-aware).

The reference generates one request at a time on ORT, copying the whole KV cache
host<->device every token (packages/lumen-vlm/src/lumen_vlm/backends/onnxrt_backend.py:
298-492).  Here one engine thread owns the device:

* requests are admitted while the native block manager can reserve
  ``prompt + max_new_tokens`` tokens (no preemption needed at 288 GB/GPU);
* each admitted request is prefilled (its ``prefill`` callable builds the input
  embeddings — vision tower + token embeddings — on the engine thread), its first
  token sampled and streamed immediately (TTFT);
* chunked prefill: a prompt longer than ``prefill_chunk`` tokens (env
  ``LUMEN_PREFILL_CHUNK``, default 2048) is prefilled ``prefill_chunk`` tokens per engine
  iteration, with a decode step of the running requests between chunks, so a long
  prompt never stalls the other streams for its whole prefill (each chunk attends the
  cached prefix: :meth:`LLM.prefill` ``prefix_blocks``);
* all running requests then advance together: one batched decode step per
  iteration (paged flash-decoding), sampling from on-device top-k candidates;
* finished sequences release their blocks;
* speculative decoding (``drafter`` / ``LUMEN_SPEC_DECODE=ngram``, off by default): when every
  running request is greedy and unpenalised and some request has a draft, the step is a verify
  step (:meth:`LLM.verify`) that scores the last token plus the draft tokens of every request and
  emits the agreeing prefix plus one token -- the same tokens in fewer steps; with
  ``spec_sampling`` / ``LUMEN_SPEC_SAMPLING=1`` sampled and penalised requests take part, every
  row's token drawn by the device sampler's verify form with the uniform of its position;
* prefix reuse (``submit(prefix_keys=...)`` / :meth:`LLMEngine.match_prefix`): a prompt whose
  leading 64-token blocks carry the content keys of an earlier prompt starts from that prompt's
  KV blocks and prefills only the rest (the chunk path above, ``start_pos`` = the hit); a prompt
  publishes its full blocks to the block manager's index once its prefill succeeded.  Not under
  tensor parallelism: with ``tp_sync`` the keys are ignored;
* guided decoding (``SamplingParams.guide``, a :class:`~lumen_amd.runtime.guided.Guide`): the request
  draws only tokens that keep its text a prefix of a match of the guide's grammar, and EOS only
  when the text is a match.  A batch with a guided request decodes through the ``guided`` graphs:
  the device sampler masks the logits by the row of the request's grammar state and advances the
  state itself, so look-ahead stays on; the host keeps the same state for the steps it feeds and
  for the host sampling path.  Such a request ends with reason ``stop`` at EOS, or ``length`` when
  ``max_new_tokens`` cuts it -- its text may then be an incomplete match.  Not under tensor
  parallelism (``submit`` raises);
* speculative decoding of guided requests (``spec_guided`` / ``LUMEN_SPEC_GUIDED=1``, off by default;
  without it a batch with a guided request takes no verify steps): a guided request drafts the
  tokens its grammar forces (:meth:`Guide.forced`: where the DFA has one live byte transition the
  continuation is known before the model runs), else the drafter's proposal cut at the first token
  the grammar does not allow.  Such a batch always takes the sampled verify form, through the
  ``verify_guided`` graphs: every row is masked by the grammar state it would be in if the draft
  tokens before it had been accepted, which the host walks and feeds.  The switch alone, without a
  drafter, speculates on the forced tokens only.

Tensor parallelism: rank 0 runs this loop and broadcasts every step (prefill inputs,
decode token ids / positions / slots / block tables) to follower ranks running
:func:`follower_loop`, so every rank issues the same kernels and collectives; only
rank 0 samples (the candidate merge makes logits identical on all ranks anyway).
"""
from __future__ import annotations

import itertools
import logging
import os
import queue
import threading
import time
from dataclasses import dataclass, field
from typing import Any, Callable, Iterator, Optional, Sequence

import numpy as np
import torch

from .. import ops
from ..ops import llm as lops
from ..parallel.comm import TPGroupUnavailable
from ..utils.h2d import h2d, h2d_ahead
from .decode_graphs import DecodeGraphs, GuideArena, SeenSlots  # noqa: F401 - also imported from here
from .kv_cache import BLOCK, PagedKVCache
from .spec_decode import Drafter, NgramDrafter, drafter_from_env, spec_tokens_from_env  # noqa: F401
from .tp_sync import TPSync, tp_sync_capacity  # noqa: F401 - also imported from here

log = logging.getLogger("lumen.engine")

# look-ahead greedy decode on the graph path (LUMEN_DECODE_LOOKAHEAD=0: one synchronous step at a time)
_LOOKAHEAD = os.environ.get("LUMEN_DECODE_LOOKAHEAD", "1") != "0"


@dataclass
class SamplingParams:
    max_new_tokens: int = 512
    temperature: float = 0.0
    top_p: float = 1.0
    repetition_penalty: float = 1.0
    stop_token_ids: tuple = ()
    seed: Optional[int] = None
    guide: Any = None                       # runtime.guided.Guide: constrain the output to its grammar


@dataclass
class GenRequest:
    rid: int
    prefill_args: Any                       # opaque, handed to the engine's prefill builder
    prompt_len: int
    params: SamplingParams
    out: "queue.Queue" = field(default_factory=queue.Queue)
    tokens: list = field(default_factory=list)
    t_submit: float = 0.0
    t_admit: Optional[float] = None         # prefill started (left the admission queue)
    t_first: Optional[float] = None
    t_done: Optional[float] = None
    finish_reason: Optional[str] = None
    ctx: int = 0                            # tokens in the KV cache
    rng: Any = None
    x: Any = None                           # prefill input embeddings while the prompt is being chunk-prefilled
    done: int = 0                           # prompt tokens prefilled so far
    cached_tokens: int = 0                  # leading prompt tokens taken from the prefix index (not computed)
    prefix_keys: Any = None                 # uint64 [n, 2] content keys of the prompt's full blocks
    seen_slot: Optional[int] = None         # in-graph sampler: row of the seen-token bitmap (penalised requests)
    seen_n: int = 0                         # ... tokens[:seen_n] are marked in it by the steps launched so far
    us: dict = field(default_factory=dict)  # ... token index -> its uniform, drawn once in token order
    u_next: int = -1                        # ... first token index whose uniform is not drawn yet
    prompt_ids: Any = None                  # speculative decoding: the prompt's token ids, if the caller gave them
    hist: Optional[list] = None             # ... prompt ids + tokens, as the drafter sees them
    hist0: int = 0                          # ... prompt ids in hist
    draft: tuple = (-1, ())                 # ... (len(tokens) it was made for, proposal)
    draft_forced: bool = False              # ... the proposal is the grammar's forced tokens (guided request)
    gstate: int = -1                        # guided decoding: the grammar state after ``tokens`` (host side)
    guide_slot: Optional[int] = None        # ... row of the device's state array
    guide_base: Optional[int] = None        # ... first arena row of the request's guide
    rope_pos: Any = None                    # multimodal RoPE: int32 [3, prompt_len] positions of the prompt (host)
    rope_delta: int = 0                     # ... RoPE position of the token at cache index c is c + rope_delta

    def stream(self, timeout: Optional[float] = None) -> Iterator[tuple]:
        """yields ("token", id) ... then ("done", reason) | raises the engine error."""
        while True:
            kind, val = self.out.get(timeout=timeout)
            if kind == "error":
                raise val
            yield kind, val
            if kind == "done":
                return


@dataclass
class PrefixHit:
    """A prefix match held for a request that is still being built: sequence ``rid`` exists in
    the block manager and shares the blocks of the first ``tokens`` prompt tokens."""
    rid: int
    tokens: int


class Sampler:
    """Greedy / temperature + nucleus sampling from per-row top-k candidates (vocab-parallel).

    ``spec`` (built on rank 0, broadcast with every TP step) carries everything that
    changes the local logits shard or the collective shapes: k, per-row 1/T and the
    repetition-penalty token sets."""

    K_SAMPLE = 64

    def __init__(self, llm):
        self.llm = llm
        self.d2h = 0          # host round trips of the candidate gather (gloo groups only)

    @staticmethod
    def spec(reqs: Sequence[GenRequest]) -> dict:
        sample = any(r.params.temperature > 0 for r in reqs)
        pens = [float(r.params.repetition_penalty) for r in reqs]
        use_pen = any(abs(p - 1.0) > 1e-6 for p in pens)
        spec = {"k": Sampler.K_SAMPLE if sample else 8,
                "inv": [1.0 / r.params.temperature if r.params.temperature > 0 else 1.0 for r in reqs] if sample else None,
                "pen": pens if use_pen else None,
                "pen_ids": [list(r.tokens) for r in reqs] if use_pen else None}
        if any(r.params.guide is not None for r in reqs):
            # guided rows: the allowed-token bitmap of the request's grammar state (host state)
            spec["allow"] = [r.params.guide.allow[r.gstate] if r.params.guide is not None else None for r in reqs]
        return spec

    def candidates(self, logits: torch.Tensor, spec: dict):
        if spec.get("allow") is not None:      # before the penalty and the 1/T, as the device sampler masks
            lops.mask_logits_(logits, spec["allow"], self.llm.v0)
        if spec["pen"] is not None:
            lops.rep_penalty_(logits, [[t - self.llm.v0 for t in ids] for ids in spec["pen_ids"]], spec["pen"])
        if spec["inv"] is not None:
            logits.mul_(h2d(spec["inv"], logits.device, torch.float32)[:, None])
        k = spec["k"]
        v, i, lse = ops.row_topk(logits, k, with_lse=True, index_offset=self.llm.v0)
        tp = self.llm.tp
        if tp.enabled:
            # ONE all-gather of the packed (values, indices, lse) rows -- vocab ids < 2^24 are exact
            # in fp32 -- and the merge (global top-k, lse of the shard lse's) on the device
            import torch.distributed as dist

            B = v.shape[0]
            packed = torch.cat([v, i.to(torch.float32), lse.view(B, 1)], 1).contiguous()
            if packed.is_cuda and dist.get_backend(tp.group) == "gloo":    # gloo gathers host tensors only
                packed = packed.cpu()
                self.d2h += 1
            parts = [torch.empty_like(packed) for _ in range(tp.world)]
            dist.all_gather(parts, packed, group=tp.group)
            allp = torch.stack(parts, 1)                                   # [B, world, 2k + 1]
            vals, ids = allp[..., :k].reshape(B, -1), allp[..., k:2 * k].reshape(B, -1)
            lse = torch.logsumexp(allp[..., 2 * k], 1)
            v, order = torch.topk(vals, k, dim=1)
            i = torch.gather(ids, 1, order).to(torch.int32)
        return v, i, lse

    def pick(self, cands, reqs: Sequence[GenRequest], uniform: Optional[Callable] = None) -> list[int]:
        """``uniform(r, n)``: the engine's per-request uniform stream.  A request that has drawn from
        it (``u_next >= 0``: a device-sampled or verify step ran) takes token n's value from there,
        by the device sampler's rule -- ``Generator.choice`` would draw a fresh one and leave the
        stream's order."""
        v, i, lse = (t.cpu().numpy() for t in cands)
        out = []
        for b, r in enumerate(reqs):
            if r.params.temperature > 0 and uniform is not None and r.u_next >= 0:
                c = np.cumsum(np.exp(v[b].astype(np.float64) - np.float64(lse[b])))
                tp = float(r.params.top_p)
                n = int(np.searchsorted(c, tp * c[-1] if c[-1] < tp else tp) + 1)
                n = max(1, min(n, len(c)))
                j = min(n - 1, int(np.searchsorted(c[:n] / c[n - 1], uniform(r, len(r.tokens)), side="right")))
                out.append(int(i[b, j]))
            elif r.params.temperature > 0:
                out.append(lops.sample_from_candidates(v[b], i[b], float(lse[b]), r.params.temperature,
                                                       r.params.top_p, r.rng))
            else:
                out.append(int(i[b, 0]))
        return out



class LLMEngine:
    def __init__(self, llm, kv: PagedKVCache, prefill_builder: Callable[[Any], torch.Tensor], max_batch: int = 64,
                 max_prefill_per_step: int = 4, tp_sync: Optional[TPSync] = None, name: str = "vlm",
                 use_graphs: Optional[bool] = None, prefill_chunk: Optional[int] = None,
                 follower_args: Optional[Callable[[Any], Any]] = None, ingraph_sampling: Optional[bool] = None,
                 spec_tokens: Optional[int] = None, drafter: Optional[Drafter] = None,
                 spec_sampling: Optional[bool] = None, spec_guided: Optional[bool] = None):
        """``follower_args``: what the TP followers receive instead of the prefill arguments
        (the VLM strips the image: only rank 0 decodes it and runs the vision tower).
        ``ingraph_sampling``: sampled / penalised requests decode through the graphs' device
        sampler with look-ahead (single GPU; None: env ``LUMEN_INGRAPH_SAMPLING``, default on).
        Off: they take the synchronous host path, as they always do under TP and without graphs.
        ``drafter`` (``callable(token_ids, k) -> list[int]``; None: env ``LUMEN_SPEC_DECODE=ngram``
        gives :class:`NgramDrafter`, default off): speculative decoding of greedy requests, with
        ``spec_tokens`` draft tokens per verify step (None: env ``LUMEN_SPEC_TOKENS``, default 3,
        1 .. 7).
        ``spec_sampling`` (None: env ``LUMEN_SPEC_SAMPLING=1``, default off): batches with sampled
        or penalised requests take verify steps too, drawn by the device sampler's verify form.
        ``spec_guided`` (None: env ``LUMEN_SPEC_GUIDED=1``, default off): batches with guided requests
        take verify steps, always in the sampled form with the sampler's guided verify form.  A guided
        request drafts its grammar's forced tokens, else what ``drafter`` proposes cut at the
        grammar; without a drafter it speculates on the forced tokens alone."""
        self.llm = llm
        self.kv = kv
        self.build = prefill_builder
        self.max_batch = max_batch
        self.max_prefill = max_prefill_per_step
        self.sync = tp_sync
        self.sampler = Sampler(llm)
        self._ids = itertools.count(1)
        self._waiting: "queue.Queue[GenRequest]" = queue.Queue()
        self._running: list[GenRequest] = []
        self._prefilling: list[GenRequest] = []
        self.prefill_chunk = max(16, int(prefill_chunk or os.environ.get("LUMEN_PREFILL_CHUNK", 2048)))
        self._stop = threading.Event()
        self._ws: dict = {}
        self._pending: Optional[tuple] = None     # (request ids, handle) of a look-ahead decode step in flight
        self.device = llm.embed.device
        self.stats = {"prefills": 0, "prefill_chunks": 0, "decode_steps": 0, "tokens": 0,
                      "prefix_hits": 0, "prefix_tokens": 0, "prefill_tokens": 0,
                      "spec_steps": 0, "spec_drafted": 0, "spec_accepted": 0, "spec_sample_steps": 0,
                      "guided_steps": 0, "spec_guided_steps": 0, "spec_forced_drafted": 0, "spec_forced_accepted": 0}
        self._arena: Optional[GuideArena] = None     # guided decoding's device tables, built on first need
        if use_graphs is None:
            use_graphs = os.environ.get("LUMEN_HIP_GRAPHS", "1") == "1"
        self.graphs: Optional[DecodeGraphs] = None
        # under TP every rank captures / replays the same decode graphs in lockstep (the leader's
        # step descriptor says when); the in-graph all-reduces are the IPC one-shot kernel or RCCL
        if use_graphs and llm.tp.enabled:
            use_graphs = os.environ.get("LUMEN_TP_GRAPHS", "1") == "1"
        if use_graphs and self.device.type == "cuda":
            self.graphs = DecodeGraphs(llm, kv, max_batch, -(-llm.cfg.max_position // 64))
        self.follower_args = follower_args
        if ingraph_sampling is None:
            ingraph_sampling = os.environ.get("LUMEN_INGRAPH_SAMPLING", "1") != "0"
        self.ingraph_sampling = bool(ingraph_sampling) and tp_sync is None and not llm.tp.enabled
        self.drafter = drafter if drafter is not None else drafter_from_env()
        self.spec_T = spec_tokens_from_env(spec_tokens) + 1      # rows per sequence of a verify step
        if spec_sampling is None:
            spec_sampling = os.environ.get("LUMEN_SPEC_SAMPLING", "0") == "1"
        self.spec_sampling = bool(spec_sampling) and tp_sync is None and not llm.tp.enabled
        if spec_guided is None:
            spec_guided = os.environ.get("LUMEN_SPEC_GUIDED", "0") == "1"
        self.spec_guided = bool(spec_guided) and tp_sync is None and not llm.tp.enabled
        # the seen-token bitmaps: the graphs' own (kept if a capture failure drops the graphs), or
        # a bare set for sampled verify steps without graphs
        self._slots: Optional[SeenSlots] = self.graphs
        if self._slots is None and self._verify_needs_slots:
            self._slots = SeenSlots(llm, max_batch)
        self._thread = threading.Thread(target=self._loop, name=f"lumen-{name}-engine", daemon=True)
        self._thread.start()

    @property
    def _verify_needs_slots(self) -> bool:
        """verify steps of this engine may take the sampled form, which penalises from the bitmap slots"""
        return (self.spec_sampling and self.drafter is not None) or self.spec_guided

    # ------------------------------------------------------------------ public API
    @staticmethod
    def _hit_cap(prompt_len: int) -> int:
        """blocks a hit may cover: the prompt's last row is always computed (it yields the logits)"""
        return max(0, (prompt_len - 1) // BLOCK)

    def match_prefix(self, prefix_keys, prompt_len: Optional[int] = None) -> PrefixHit:
        """Match ``prefix_keys`` (uint64 [n, 2], one chained content key per full 64-token block
        of a prompt) against the prefix index under a fresh request id and hold the matched
        blocks.  Pass the hit to :meth:`submit` (``hit=``) or give it back with
        :meth:`release_prefix`.  ``prompt_len`` caps the hit so that the last row is computed.
        Tensor parallelism: no reuse, the hit is empty."""
        rid = next(self._ids)
        if prefix_keys is None or self.sync is not None:
            return PrefixHit(rid, 0)
        keys = np.ascontiguousarray(prefix_keys, dtype=np.uint64).reshape(-1, 2)
        if prompt_len is not None:
            keys = keys[:self._hit_cap(prompt_len)]
        return PrefixHit(rid, self.kv.blocks.match(keys, rid))

    def release_prefix(self, hit: Optional[PrefixHit]) -> None:
        """Drop the references of a hit whose request is abandoned before submit."""
        if hit is not None and hit.tokens > 0:
            self.kv.blocks.release(hit.rid)
            hit.tokens = 0

    def submit(self, prefill_args: Any, prompt_len: int, params: SamplingParams, prefix_keys=None,
               hit: Optional[PrefixHit] = None, prompt_ids: Optional[Sequence[int]] = None,
               rope_pos=None) -> GenRequest:
        """``prefix_keys``: uint64 [n, 2], key i covering prompt tokens [64 i, 64 i + 64) and chaining
        key i - 1 -- the prompt may start from cached blocks and publishes its own after prefill.
        ``hit``: the result of an earlier :meth:`match_prefix` with the same keys (the request
        takes over its id and references).  The prefill builder must return all ``prompt_len``
        rows; rows before the hit are never read.
        ``prompt_ids``: the prompt's token ids for the speculative-decoding drafter (without them
        it sees the generated tokens only).
        ``rope_pos``: int32 [3, prompt_len] multimodal-RoPE positions of the prompt (a decoder with
        ``cfg.mrope``; ``VLM.rope_positions``).  Prefill chunks rotate with their columns; generated
        tokens with cache index + delta, delta = max(rope_pos) + 1 - prompt_len."""
        try:
            if self._stop.is_set():
                raise RuntimeError("engine stopped")
            rope_delta = 0
            if rope_pos is not None:
                rope_pos, rope_delta = self._check_rope_pos(rope_pos, prompt_len, params)
            need = prompt_len + params.max_new_tokens
            if need > self.kv.capacity_tokens:
                raise ValueError(f"request needs {need} KV tokens, cache holds {self.kv.capacity_tokens}")
            if params.guide is not None:
                if self.sync is not None or self.llm.tp.enabled:
                    raise ValueError("guided decoding is not supported under tensor parallelism")
                if params.guide.V > self.llm.Vl:
                    raise ValueError(f"the guide covers {params.guide.V} tokens, the model's vocabulary {self.llm.Vl}")
        except Exception:
            self.release_prefix(hit)
            raise
        if prompt_len + params.max_new_tokens > self.llm.cfg.max_position:
            params.max_new_tokens = max(1, self.llm.cfg.max_position - prompt_len)
        keys = None
        if prefix_keys is not None and self.sync is None:
            keys = np.ascontiguousarray(prefix_keys, dtype=np.uint64).reshape(-1, 2)[:prompt_len // BLOCK]
        if hit is None:
            hit = self.match_prefix(keys, prompt_len)
        elif hit.tokens > self._hit_cap(prompt_len) * BLOCK:
            # matched without the prompt length: give the last block back
            self.release_prefix(hit)
            if keys is not None:
                hit.tokens = self.kv.blocks.match(keys[:self._hit_cap(prompt_len)], hit.rid)
        r = GenRequest(rid=hit.rid, prefill_args=prefill_args, prompt_len=prompt_len, params=params,
                       t_submit=time.perf_counter(), rng=np.random.default_rng(params.seed),
                       cached_tokens=hit.tokens, prefix_keys=keys, prompt_ids=prompt_ids, rope_pos=rope_pos,
                       rope_delta=rope_delta)
        if params.guide is not None:
            r.gstate = params.guide.start
        self._waiting.put(r)
        return r

    def _check_rope_pos(self, rope_pos, prompt_len: int, params: SamplingParams) -> tuple:
        """-> (int32 [3, prompt_len] on the host, rope delta) of a request's multimodal-RoPE positions"""
        cfg = self.llm.cfg
        if self.sync is not None or self.llm.tp.enabled:
            raise ValueError("rope_pos (multimodal RoPE) is not supported under tensor parallelism")
        if cfg.mrope is None:
            raise ValueError("rope_pos given for a decoder without multimodal RoPE")
        p = np.asarray(rope_pos.cpu() if isinstance(rope_pos, torch.Tensor) else rope_pos)
        if p.shape != (3, prompt_len) or not np.issubdtype(p.dtype, np.integer):
            raise ValueError(f"rope_pos: int32 [3, {prompt_len}] expected, got {p.dtype} {list(p.shape)}")
        if prompt_len == 0 or int(p.min()) < 0:
            raise ValueError("rope_pos: positions must be >= 0")
        top = int(p.max()) + 1
        new = min(params.max_new_tokens, max(1, cfg.max_position - prompt_len))     # as submit clips it
        if top + new > cfg.max_position:
            raise ValueError(f"rope_pos: positions up to {top - 1} + {new} new tokens exceed max_position "
                             f"{cfg.max_position}")
        return torch.from_numpy(np.ascontiguousarray(p, dtype=np.int32)), top - prompt_len

    def close(self) -> None:
        self._stop.set()
        self._thread.join(timeout=10)
        if self.sync is not None:
            try:
                self.sync.send(("stop",))
            except Exception:  # pragma: no cover
                pass
            self.sync.close()

    # ------------------------------------------------------------------ loop
    def _emit(self, r: GenRequest, tok: int) -> bool:
        """record token; returns True when the request finished."""
        p = r.params
        if p.guide is not None:
            # the host's copy of the grammar state: what a fed step and the host sampling path mask by
            if not p.guide.allows(r.gstate, tok):
                raise RuntimeError(f"guided decoding: token {tok} is not allowed in grammar state {r.gstate}")
            if tok in p.stop_token_ids or tok in p.guide.eos_ids:     # EOS: only allowed in an accepting state
                r.finish_reason = "stop"
                return True
            r.gstate = p.guide.walk(r.gstate, tok)
        if tok in p.stop_token_ids:
            r.finish_reason = "eos_token"
            return True
        r.tokens.append(tok)
        r.out.put(("token", tok))
        self.stats["tokens"] += 1
        if len(r.tokens) >= p.max_new_tokens:
            r.finish_reason = "length"
            return True
        return False

    def _advance(self, reqs, toks) -> list:
        """The step's outcome: request i takes ``toks[i]`` in order (one token of a decode step, the
        accepted rows' tokens of a verify step), each advancing its context, up to the first that
        finishes it.  The requests that go on are the running batch, which is returned."""
        still = []
        for r, ts in zip(reqs, toks):
            for t in ts:
                r.ctx += 1
                if self._emit(r, int(t)):
                    self._finish(r)
                    break
            else:
                still.append(r)
        self._running = still
        return still

    @staticmethod
    def _penalised(r: GenRequest) -> bool:
        return abs(float(r.params.repetition_penalty) - 1.0) > 1e-6

    def _join(self, r: GenRequest) -> None:
        """``r`` enters the running batch; a penalised request takes a zeroed row of the device
        sampler's seen bitmap (none free, or no graphs: its batches sample on the host)"""
        wanted = (self.ingraph_sampling and self.graphs is not None) or \
            (self._verify_needs_slots and self._slots is not None)
        if wanted and self._penalised(r):
            r.seen_slot = self._slots.take_slot()
            if r.seen_slot is not None:
                self._slots.write_slot(r.seen_slot, r.tokens[:-1])
                r.seen_n = len(r.tokens) - 1
        self._running.append(r)

    def _guide_acquire(self, r: GenRequest) -> None:
        """a guided request that may decode through the ``guided`` graphs, or take guided verify steps
        (``spec_guided``, with or without graphs), takes its guide's arena rows (uploading the guide on
        first use) and a row of the device's grammar states.  A guide that does not fit raises
        GuideError: the caller fails this request only."""
        g = r.params.guide
        if g is None or r.guide_base is not None:
            return
        if not self.spec_guided and (self.graphs is None or not self.ingraph_sampling or not _LOOKAHEAD):
            return
        if self._arena is None:
            self._arena = GuideArena(self.llm, self.max_batch, g.token_bytes)
        if self.graphs is not None:
            self.graphs.arena = self._arena
        r.guide_base = self._arena.acquire(g)
        r.guide_slot = self._arena.take_slot()

    def _drop_slot(self, r: GenRequest) -> None:
        if r.seen_slot is not None and self._slots is not None:
            self._slots.free_slot(r.seen_slot)
        r.seen_slot = None
        if r.guide_base is not None and self._arena is not None:
            self._arena.release(r.params.guide)
            if r.guide_slot is not None:
                self._arena.free_slot(r.guide_slot)
        r.guide_base = r.guide_slot = None

    def _finish(self, r: GenRequest) -> None:
        self._drop_slot(r)
        self.kv.blocks.release(r.rid)
        r.t_done = time.perf_counter()
        r.out.put(("done", r.finish_reason or "stop"))

    def _fail(self, reqs, e: BaseException) -> None:
        for r in reqs:
            self._drop_slot(r)
            try:
                self.kv.blocks.release(r.rid)
            except Exception:
                pass
            r.out.put(("error", e))

    def cancel(self, r: GenRequest) -> None:
        r.params.max_new_tokens = len(r.tokens)   # finishes at the next step

    def _admit(self) -> list[GenRequest]:
        adm = []
        while (len(self._running) + len(self._prefilling) + len(adm) < self.max_batch
               and len(self._prefilling) + len(adm) < self.max_prefill):
            try:
                r = self._waiting.get_nowait()
            except queue.Empty:
                break
            if not self.kv.blocks.reserve(r.rid, r.prompt_len + r.params.max_new_tokens):
                self._waiting.put(r)   # retry when blocks free up
                break
            adm.append(r)
        return adm

    @torch.no_grad()
    def _prefill_chunk(self, r: GenRequest, budget: int) -> int:
        """Prefill up to ``budget`` more prompt tokens of ``r``; returns the tokens consumed.
        On the last chunk the first token is sampled and ``r`` joins the running batch."""
        if r.x is None:
            if r.t_admit is None:
                r.t_admit = time.perf_counter()
            self._guide_acquire(r)
            if self.sync is not None:
                # followers must enter the build (its vocab-parallel embedding all-reduce)
                # together with us: announce it before building the inputs
                fa = self.follower_args(r.prefill_args) if self.follower_args is not None else r.prefill_args
                self.sync.send(("pbuild", r.rid, fa))
                x = self.build(r.prefill_args)
                if x.shape[0] != r.prompt_len:
                    raise RuntimeError(f"prefill built {x.shape[0]} rows for a {r.prompt_len}-token prompt")
            else:
                x = self.build(r.prefill_args)
                if r.cached_tokens and x.shape[0] != r.prompt_len:
                    raise RuntimeError(f"prefill built {x.shape[0]} rows for a {r.prompt_len}-token prompt "
                                       f"with {r.cached_tokens} cached tokens")
                r.prompt_len = x.shape[0]
            r.x, r.done = x, r.cached_tokens
            if r.cached_tokens:
                self.stats["prefix_hits"] += 1
                self.stats["prefix_tokens"] += r.cached_tokens
        T = r.prompt_len
        s = r.done
        e = min(T, s + max(1, budget))
        last = e == T
        slots = self.kv.slots(r.rid, s, e - s)
        tab = np.asarray(self.kv.blocks.table(r.rid), np.int64)[: -(-e // BLOCK)] if s > 0 else None
        spec = Sampler.spec([r]) if last else None
        if self.sync is not None:
            self.sync.send(("pchunk", r.rid, s, e, slots, tab, spec, last))
        pos3 = {}
        if r.rope_pos is not None:
            if r.rope_pos.shape[1] != T:
                raise RuntimeError(f"rope_pos covers {r.rope_pos.shape[1]} tokens, the prefill built {T} rows")
            pos3 = {"pos3": h2d(r.rope_pos[:, s:e].contiguous(), self.device)}
        logits = self.llm.prefill(r.x[s:e], self.kv, h2d_ahead(slots, self.device), start_pos=s,
                                  prefix_blocks=h2d_ahead(tab, self.device) if tab is not None else None, **pos3)
        r.done = e
        self.stats["prefill_chunks"] += 1
        self.stats["prefill_tokens"] += e - s
        if not last:
            return e - s
        r.x = None
        r.ctx = T
        tok = self.sampler.pick(self.sampler.candidates(logits, spec), [r])[0]
        r.t_first = time.perf_counter()
        # the whole prompt is in the cache (the token read above waited for it): its full blocks
        # become matchable.  Later requests run on this stream too, so they read after these writes.
        if r.prefix_keys is not None and len(r.prefix_keys):
            self.kv.blocks.publish(r.rid, r.prefix_keys[:T // BLOCK])
        self.stats["prefills"] += 1
        self._prefilling.remove(r)
        if self._emit(r, tok):
            self._finish(r)
        else:
            self._join(r)
        return e - s

    def _prefill_round(self) -> None:
        """One engine iteration's prefill work: up to ``prefill_chunk`` prompt tokens,
        oldest request first.  (Packing several prompts into one forward measured neutral for
        Llama-3-8B fp8 and slower for FastVLM-0.5B batch 16, profiles/r2_prefill_pack_v1.txt,
        so chunks run per request.)"""
        budget = self.prefill_chunk
        for r in list(self._prefilling):
            if budget <= 0:
                break
            try:
                budget -= self._prefill_chunk(r, budget)
            except Exception as e:  # noqa: BLE001 - surfaced to the caller
                log.exception("prefill failed")
                if r in self._prefilling:
                    self._prefilling.remove(r)
                r.x = None
                self._fail([r], e)

    def _greedy_graph_ok(self, reqs, spec) -> bool:
        """the in-graph greedy sampler serves this step: graphs on, every request greedy without
        repetition penalty, batch and table within the graph buckets (any TP size)"""
        g = self.graphs
        return (g is not None and g.in_graph_sampler and _LOOKAHEAD
                and spec["inv"] is None and spec["pen"] is None and spec["k"] <= g.K_GREEDY
                and spec.get("allow") is None and len(reqs) <= g.buckets[-1])

    def _guided_graph_ok(self, reqs, spec) -> bool:
        """the ``guided`` graphs serve this step: what the device sampler needs, and every guided
        request holds its guide's arena rows and a row of the device's grammar states"""
        return (self._sample_graph_ok(reqs, spec) and self._arena is not None
                and all(r.guide_base is not None and r.guide_slot is not None
                        for r in reqs if r.params.guide is not None))

    def _sample_graph_ok(self, reqs, spec) -> bool:
        """the in-graph device sampler serves this step: single GPU, graphs and look-ahead on, at
        most 64 candidates per row, and every penalised request holds a bitmap slot"""
        g = self.graphs
        return (self.ingraph_sampling and g is not None and _LOOKAHEAD and spec["k"] <= Sampler.K_SAMPLE
                and len(reqs) <= g.buckets[-1] and self.llm.Vl >= lops.SAMPLE_K
                and all(r.seen_slot is not None for r in reqs if self._penalised(r)))

    def _uniform(self, r: GenRequest, n: int, base: Optional[int] = None) -> float:
        """the uniform of token ``n`` of ``r``: ``r.rng.random()``, which is what the host path's
        ``Generator.choice`` draws for it -- once, in token order, kept for a step that is launched
        again after a discarded look-ahead or that follows a verify step whose rows drew ahead
        (``base``: the first token of such a step; values from ``base - 1`` on are kept)"""
        if r.params.temperature <= 0:
            return 0.0
        if r.u_next < 0:
            r.u_next = len(r.tokens)          # the tokens so far were sampled on the host
        while r.u_next <= n:
            r.us[r.u_next] = float(r.rng.random())
            r.u_next += 1
        lo = (n if base is None else base) - 1
        for k in [k for k in r.us if k < lo]:
            del r.us[k]
        return r.us[n]

    @staticmethod
    def _sampler_rows(reqs) -> dict:
        """the device sampler's per-sequence inputs (a penalised request without a bitmap slot is not
        penalised: such a batch never gets here)"""
        ps = [r.params for r in reqs]
        return {"inv_t": np.array([1.0 / p.temperature if p.temperature > 0 else 1.0 for p in ps], np.float32),
                "top_p": np.array([p.top_p for p in ps], np.float64),
                "penalty": np.array([float(p.repetition_penalty) if r.seen_slot is not None else 1.0
                                     for p, r in zip(ps, reqs)], np.float32),
                "greedy": np.array([p.temperature <= 0 for p in ps], np.int32),
                "seen_slot": np.array([-1 if r.seen_slot is None else r.seen_slot for r in reqs], np.int32)}

    def _sample_inputs(self, reqs, ahead: int, fed: bool, guided: bool = False) -> dict:
        """per-row inputs of the device sampler for the step that yields token len(tokens) + ahead;
        ``fed``: the step gets its input tokens from the host (not a look-ahead); ``guided``: the
        step runs the ``guided`` graph and also carries the rows' grammar-state slots and states"""
        for r in reqs:
            if r.seen_slot is None:
                continue
            n = len(r.tokens)
            if fed:
                if r.seen_n not in (n - 1, n):    # steps of this request ran elsewhere: rebuild its row
                    self._slots.write_slot(r.seen_slot, r.tokens[:-1])
                r.seen_n = n                      # this step marks tokens[-1]
            else:
                r.seen_n = n + 1                  # ... and this one the token the step before it draws
        out = self._sampler_rows(reqs)
        out["u"] = np.array([self._uniform(r, len(r.tokens) + ahead) for r in reqs], np.float64)
        if guided:
            # a fed step carries the state the host derived from the request's tokens; a look-ahead
            # step reads the one the step before it stored, so a discarded look-ahead step that is
            # launched again as a fed step cannot advance the state twice
            gd = [r.params.guide is not None for r in reqs]
            out["g_slot"] = np.array([r.guide_slot if g else -1 for r, g in zip(reqs, gd)], np.int32)
            out["g_in"] = np.array([r.guide_base + r.gstate if g and fed else -1 for r, g in zip(reqs, gd)], np.int32)
        return out

    def _graphs_failed(self, e: BaseException) -> None:
        """a capture or replay failed: eager launches from now on.  Not under TP, where the ranks
        must not diverge: the error is raised instead of falling back"""
        if self.sync is not None:
            raise e
        log.warning("hipGraph decode disabled: %s", e)
        self.graphs = None

    def _graph_ready(self, reqs, mode: str = "greedy") -> bool:
        """the step's graph exists or captures now (a capture failure disables graphs).  Under
        TP the capture runs collectives, so it happens inside the launch, after the followers
        received the step (they capture the same graph at the same point)."""
        w = max(len(self.kv.blocks.table(r.rid)) for r in reqs)
        if w > self.graphs.max_blocks:
            return False
        if self.sync is not None:
            return True
        try:
            self.graphs.ensure(len(reqs), w, mode)
            return True
        except Exception as e:  # noqa: BLE001 - capture unsupported
            self._graphs_failed(e)
            return False

    def _step_inputs(self, reqs, ahead: int):
        """positions / slots / block table / context lengths of the step that feeds cache index
        r.ctx + ahead of every request (its RoPE position: the index + the request's rope delta)"""
        idx = np.array([r.ctx + ahead for r in reqs], np.int32)
        pos = idx + np.array([r.rope_delta for r in reqs], np.int32)
        slots = np.concatenate([self.kv.slots(r.rid, r.ctx + ahead, 1) for r in reqs])
        bt = self.kv.block_table([r.rid for r in reqs])
        return pos, slots, bt, idx + 1

    def _can_look_ahead(self, reqs) -> bool:
        """every request surely runs one more step after this one (no length finish, its reserved
        blocks cover the next position) and nothing waits to join the batch"""
        if self._prefilling or not self._waiting.empty():
            return False
        for r in reqs:
            if len(r.tokens) + 1 >= r.params.max_new_tokens:
                return False
            if len(self.kv.blocks.table(r.rid)) * BLOCK <= r.ctx + 1:
                return False
        return True

    # ------------------------------------------------------------------ speculative decoding
    def _spec_ok(self, reqs) -> bool:
        """a verify step may serve this batch: a drafter is set, single GPU without a step channel,
        every request greedy without repetition penalty, and B * T rows fit the 32-row decode GEMMs.
        With ``spec_sampling`` sampled and penalised requests may take part: the vocabulary holds the
        sampler's 64 candidates and every penalised request holds a bitmap slot.
        A batch with a guided request takes verify steps only with ``spec_guided`` (a drafter is not
        needed then: the grammar's forced tokens are a draft), always in the sampled form, whatever
        ``spec_sampling`` says -- a greedy guided request needs the mask too -- so the sampled form's
        conditions hold and every guided request holds its guide's arena rows"""
        guided = self._spec_guided(reqs)
        if not ((self.drafter is not None or (guided and self.spec_guided)) and self.sync is None
                and not self.llm.tp.enabled and len(reqs) * self.spec_T <= 32):
            return False
        if guided and not (self.spec_guided and self._arena is not None
                           and all(r.guide_base is not None for r in reqs if r.params.guide is not None)):
            return False      # without the switch guided requests take no verify steps
        if not guided and not self._spec_sampled(reqs):
            return True
        return ((guided or self.spec_sampling) and self._slots is not None and self.llm.Vl >= lops.SAMPLE_K
                and self.spec_T <= lops.SAMPLE_VERIFY_MAX_T
                and all(r.seen_slot is not None for r in reqs if self._penalised(r)))

    @staticmethod
    def _spec_guided(reqs) -> bool:
        """some request is guided: a verify step of this batch is the guided (sampled) form"""
        return any(r.params.guide is not None for r in reqs)

    def _spec_sampled(self, reqs) -> bool:
        """some request is sampled or penalised: a verify step of this batch is the sampled form"""
        return any(r.params.temperature > 0 or self._penalised(r) for r in reqs)

    def _draft(self, r: GenRequest) -> tuple:
        """the drafter's proposal for ``r``'s next tokens, cut so that the request neither exceeds
        ``max_new_tokens`` (the step also yields one token of its own) nor leaves its reserved blocks;
        made once per generated length.  A guided request (only drafted with ``spec_guided``) proposes
        the tokens its grammar forces from the host's state ``r.gstate``; where nothing is forced, the
        drafter's proposal cut at the first token the grammar does not allow in the state reached so
        far -- so every row of the verify step has a valid grammar state, which the host knows"""
        n = len(r.tokens)
        if r.draft[0] == n:
            return r.draft[1]
        k = min(self.spec_T - 1, r.params.max_new_tokens - n - 1,
                len(self.kv.blocks.table(r.rid)) * BLOCK - r.ctx - 1)
        d: tuple = ()
        g = r.params.guide
        r.draft_forced = False
        if k > 0 and g is not None:
            d = g.forced(r.gstate, k)
            r.draft_forced = bool(d)
        if k > 0 and not d and self.drafter is not None:
            if r.hist is None:
                r.hist = [int(t) for t in r.prompt_ids] if r.prompt_ids is not None else []
                r.hist0 = len(r.hist)
            r.hist.extend(r.tokens[len(r.hist) - r.hist0:])
            d = tuple(int(t) for t in self.drafter(r.hist, k))[:k]
            if g is not None:
                st, ok = r.gstate, 0
                while ok < len(d) and g.allows(st, d[ok]):
                    st = g.walk(st, d[ok])
                    ok += 1
                d = d[:ok]
        r.draft = (n, d)
        return d

    def _spec_drafts(self, reqs) -> Optional[list]:
        """per-request drafts if the next step of ``reqs`` is a verify step (some draft is non-empty)"""
        if not self._spec_ok(reqs):
            return None
        drafts = [self._draft(r) for r in reqs]
        return drafts if any(drafts) else None

    def _verify_sample_inputs(self, reqs) -> dict:
        """per-sequence inputs of the sampler's verify form and one uniform per row: row i of a
        request yields its token len(tokens) + i.  Brings every bitmap slot to tokens[:-1] (a slot
        that also holds tokens[-1], marked by a discarded look-ahead step, is as good: row 0
        penalises that token anyway and the accept kernel marks it)."""
        T = self.spec_T
        for r in reqs:
            n = len(r.tokens)
            if r.seen_slot is not None and r.seen_n not in (n - 1, n):
                self._slots.write_slot(r.seen_slot, r.tokens[:-1])
                r.seen_n = n - 1
        out = self._sampler_rows(reqs)
        out["u"] = np.array([self._uniform(r, len(r.tokens) + i, len(r.tokens)) for r in reqs for i in range(T)],
                            np.float64)
        return out

    @torch.no_grad()
    def _verify(self, reqs, drafts) -> None:
        """One verify step: sequence b feeds tokens[-1] and its draft as rows b*T .. at positions
        ctx ..; row i's arg-max is the model's token after row i's input, so draft i is accepted while
        it equals the arg-max of row i - 1, and the arg-maxes of rows 0 .. (accepted) are emitted.
        Rejected rows' cache entries lie beyond the new ctx and are rewritten when next fed.

        A batch with a sampled or penalised request takes the sampled form: row i's token is drawn by
        the device sampler's verify form from the row's penalised, scaled logits with the uniform of
        token len(tokens) + i -- what a decode step at that position would draw -- and the rule above
        holds with "drawn token" for "arg-max".  The accept kernel marks the accepted inputs in the
        bitmap slots; the uniforms of rejected rows stay stored for their positions.

        A batch with a guided request (``spec_guided``) takes the sampled form with the sampler's guided
        verify form: row i of a guided request is masked by the grammar state after the request's text
        and its draft tokens 1 .. i, which the host walks here and feeds as ``g_in``; the unguided rows
        ride along with -1.  :meth:`_emit` then walks ``r.gstate`` over the emitted tokens as ever and
        raises if one is not allowed."""
        T, B = self.spec_T, len(reqs)
        gd = self._spec_guided(reqs)
        smp = gd or self._spec_sampled(reqs)
        ids = np.zeros(B * T, np.int64)
        pos = np.zeros(B * T, np.int32)
        slots = np.full(B * T, -1, np.int64)
        n_rows = np.array([1 + len(d) for d in drafts], np.int32)
        ctx = np.array([r.ctx for r in reqs], np.int32) + n_rows
        for b, (r, d) in enumerate(zip(reqs, drafts)):
            n, o = 1 + len(d), b * T
            ids[o] = r.tokens[-1]
            ids[o + 1:o + n] = d
            pos[o:o + n] = r.ctx + r.rope_delta + np.arange(n)
            slots[o:o + n] = self.kv.slots(r.rid, r.ctx, n)
        bt = self.kv.block_table([r.rid for r in reqs])
        sample = self._verify_sample_inputs(reqs) if smp else None
        g_in = None
        if gd:
            g_in = np.full(B * T, -1, np.int32)
            for b, (r, d) in enumerate(zip(reqs, drafts)):
                g, st = r.params.guide, r.gstate
                if g is None:
                    continue
                for i in range(1 + len(d)):
                    if i:
                        st = g.walk(st, d[i - 1])
                    g_in[b * T + i] = r.guide_base + st
            sample["g_in"] = g_in
        am = n_acc = None
        if self.graphs is not None and bt.shape[1] <= self.graphs.max_blocks:
            try:
                h = self.graphs.launch_verify(ids, pos, slots, bt, ctx, n_rows, T, sample)
                am = self.graphs.verified(h)
                n_acc = h.get("n_acc")
            except Exception as e:  # noqa: BLE001 - capture unsupported
                self._graphs_failed(e)
                if smp:       # the failed launch may have left the bitmap rows anywhere
                    for r in reqs:
                        r.seen_n = -1
                    sample = self._verify_sample_inputs(reqs)
                    if gd:
                        sample["g_in"] = g_in
        if am is None:
            d = self.device
            logits = self.llm.verify(h2d(ids, d), h2d(pos, d), h2d(slots, d), self.kv, h2d(bt, d), h2d(ctx, d),
                                     h2d(n_rows, d), T, workspace=self._ws)
            if smp:
                t = lambda k, dt: h2d(sample[k], d, dt)  # noqa: E731
                # guided: the verify form reads g_in alone; the slot argument of the tensors is not read
                *_, tok, acc, _seen = lops.sample_verify_rows(
                    logits, T, h2d(n_rows, d), t("inv_t", torch.float32), t("top_p", torch.float64),
                    t("penalty", torch.float32), t("u", torch.float64), t("greedy", torch.int32),
                    t("seen_slot", torch.int32), self._slots._seen(), h2d(ids, d), candidates=False,
                    guide=self._arena.tensors(t("g_in", torch.int32), t("g_in", torch.int32)) if gd else None)
                am, n_acc = tok.cpu().numpy(), acc.cpu().numpy()
            else:
                _v, i, _lse = ops.row_topk(logits, DecodeGraphs.K_GREEDY, with_lse=True, index_offset=self.llm.v0)
                am = i[:, 0].cpu().numpy()
        self.stats["spec_steps"] += 1
        self.stats["spec_sample_steps"] += smp and not gd
        self.stats["spec_guided_steps"] += gd
        acc = []
        for b, d in enumerate(drafts):
            j = 0
            while j < len(d) and d[j] == int(am[b * T + j]):
                j += 1
            acc.append(j)
        if n_acc is not None and acc != [int(x) for x in n_acc[:B]]:      # before anything is emitted
            raise RuntimeError(f"verify step: the device accepted {list(n_acc[:B])} draft tokens, the host {acc}")
        for r, d, j in zip(reqs, drafts, acc):
            if smp:
                r.seen_n = len(r.tokens) + j      # the accept kernel marked tokens[-1] and the accepted draft tokens
            self.stats["spec_drafted"] += len(d)
            self.stats["spec_accepted"] += j
            if r.draft_forced:
                self.stats["spec_forced_drafted"] += len(d)
                self.stats["spec_forced_accepted"] += j
        self._advance(reqs, [am[b * T:b * T + j + 1] for b, j in enumerate(acc)])

    @torch.no_grad()
    def _decode(self) -> None:
        reqs = self._running
        B = len(reqs)
        # a look-ahead step in flight for this batch is consumed below by the usual rules; otherwise a
        # batch with a draft takes a verify step
        if self._pending is None or self._pending[0] != [r.rid for r in reqs]:
            drafts = self._spec_drafts(reqs)
            if drafts is not None:
                self._pending = None
                self._verify(reqs, drafts)
                return
        spec = Sampler.spec(reqs)
        if spec.get("allow") is not None:      # a batch with a guided request: the guided graphs or the host path
            mode = "guided" if self._guided_graph_ok(reqs, spec) else None
        else:
            mode = "greedy" if self._greedy_graph_ok(reqs, spec) else "sample" if self._sample_graph_ok(reqs, spec) \
                else None
        if mode is not None and self._graph_ready(reqs, mode):
            # look-ahead decode: the step after this one is launched (token ids taken from this
            # step's in-graph arg-max or draw) BEFORE this step's tokens are read, so the host work of
            # reading, streaming and scheduling overlaps the GPU instead of idling it between steps
            rids = [r.rid for r in reqs]
            gd = mode == "guided"
            smp = mode == "sample" or gd      # the mode follows from the requests, so a pending step has the same
            pend, self._pending = self._pending, None
            if pend is not None and pend[0] == rids:
                h = pend[1]
            else:
                ids = np.array([r.tokens[-1] for r in reqs], np.int64)
                h = self._launch_greedy(ids, self._step_inputs(reqs, 0), spec,
                                        self._sample_inputs(reqs, 0, True, gd) if smp else None)
            nxt = None
            # with a drafter the next step may be a verify step, known only once this step's tokens
            # are read: the look-ahead is then launched after them, and only if nothing was drafted
            late = self._spec_ok(reqs)
            if not late and self._can_look_ahead(reqs):
                nxt = self._launch_greedy(None, self._step_inputs(reqs, 1), spec,
                                          self._sample_inputs(reqs, 1, False, gd) if smp else None)
            if smp:
                toks = [int(t) for t in self.graphs.sampled(h)]
                self.stats["guided_steps" if gd else "ingraph_sample_steps"] = \
                    self.stats.get("guided_steps" if gd else "ingraph_sample_steps", 0) + 1
            else:
                _v, i, _lse = self.graphs.tokens(h)
                toks = [int(i[b, 0]) for b in range(B)]
            if h.get("err"):
                # an IPC all-reduce of this step gave up on a peer: its tokens are garbage
                self._pending = None
                raise TPGroupUnavailable("tensor-parallel peer not responding (IPC all-reduce timed out)")
            self.stats["decode_steps"] += 1
            still = self._advance(reqs, [(t,) for t in toks])
            if late and len(still) == B and self._can_look_ahead(reqs) and self._spec_drafts(reqs) is None:
                nxt = self._launch_greedy(np.array([r.tokens[-1] for r in reqs], np.int64),
                                          self._step_inputs(reqs, 0), spec,      # ctx already advanced
                                          self._sample_inputs(reqs, 0, True, gd) if smp else None)
            if nxt is not None and len(still) == B:
                self._pending = (rids, nxt)
                self.stats["lookahead_steps"] = self.stats.get("lookahead_steps", 0) + 1
            return
        self._pending = None
        ids = np.array([r.tokens[-1] for r in reqs], np.int64)
        pos, slots, bt, ctx = self._step_inputs(reqs, 0)
        graph = self.graphs is not None and bt.shape[1] <= self.graphs.max_blocks
        if self.sync is not None:
            self.sync.send_decode(ids, pos, slots, bt, ctx, spec, graph)
        logits = self._decode_step(ids, pos, slots, bt, ctx, graph)
        toks = self.sampler.pick(self.sampler.candidates(logits, spec), reqs, self._uniform)
        self.stats["decode_steps"] += 1
        comm = getattr(self.llm, "comm", None)
        if comm is not None:
            comm.check()    # before emitting; the tokens' D2H already waited for the step
        self._advance(reqs, [(t,) for t in toks])

    def _launch_greedy(self, ids, inputs, spec, sample: Optional[dict] = None) -> dict:
        """One in-graph-sampled step (``ids`` None: look-ahead, ids from the device); under TP the
        followers get the descriptor first and replay the same graph.  ``sample``: the device
        sampler's per-row inputs (single GPU) instead of the greedy arg-max."""
        if self.sync is not None:
            self.sync.send_decode(ids, *inputs, spec, graph=True, ingraph=True)
        try:
            return self.graphs.launch(ids, *inputs, sample=sample)
        except Exception as e:
            self._graphs_failed(e)
            raise

    def _decode_step(self, ids, pos, slots, bt, ctx, graph: bool = True) -> torch.Tensor:
        d = self.device
        if graph and self.graphs is not None and bt.shape[1] <= self.graphs.max_blocks:
            try:
                return self.graphs.run(ids, pos, slots, bt, ctx)
            except Exception as e:  # noqa: BLE001 - capture unsupported: fall back to eager launches
                self._graphs_failed(e)
        return self.llm.decode(h2d(ids, d), h2d(pos, d), h2d(slots, d), self.kv, h2d(bt, d), h2d(ctx, d),
                               workspace=self._ws)

    def _loop(self) -> None:
        if self.device.type == "cuda":
            torch.cuda.set_device(self.device)
        while not self._stop.is_set():
            self._prefilling.extend(self._admit())
            if not self._prefilling and not self._running:
                try:
                    r = self._waiting.get(timeout=0.05)
                    self._waiting.put(r)
                except queue.Empty:
                    pass
                continue
            if self._prefilling:
                self._prefill_round()
            if self._running:
                try:
                    self._decode()
                except Exception as e:  # noqa: BLE001
                    log.exception("decode step failed")
                    self._fail(self._running, e)
                    self._running = []
                    self._pending = None


def follower_loop(llm, kv: PagedKVCache, prefill_builder: Callable[[Any], torch.Tensor], sync: TPSync,
                  max_batch: int = 64) -> dict:
    """Non-zero TP ranks: replay rank 0's steps so every collective is matched.  Greedy decode
    steps (flag ``ingraph``) are a descriptor read from the step bus + one graph launch: the
    graph samples on the device, so the follower never reads a result back.  Returns the
    follower's counters (also written as JSON to ``$LUMEN_TP_FOLLOWER_STATS`` when set)."""
    sampler = Sampler(llm)
    ws: dict = {}
    xs: dict = {}                            # rid -> prefill embeddings of prompts being chunk-prefilled
    dev = llm.embed.device
    graphs = None
    if dev.type == "cuda" and os.environ.get("LUMEN_HIP_GRAPHS", "1") == "1" and \
            os.environ.get("LUMEN_TP_GRAPHS", "1") == "1":
        graphs = DecodeGraphs(llm, kv, max_batch, -(-llm.cfg.max_position // 64))   # the leader's buckets
    stats = {"decode_steps": 0, "ingraph_steps": 0, "lookahead_steps": 0, "prefill_chunks": 0}
    while True:
        msg = sync.recv()
        kind = msg[0]
        if kind == "stop":
            break
        with torch.no_grad():
            if kind == "pbuild":
                _, rid, args = msg
                xs[rid] = prefill_builder(args)
            elif kind == "pchunk":
                _, rid, s, e, slots, tab, spec, last = msg
                x = xs[rid] if not last else xs.pop(rid)
                logits = llm.prefill(x[s:e], kv, h2d(slots, dev), start_pos=s,
                                     prefix_blocks=h2d(tab, dev) if tab is not None else None)
                stats["prefill_chunks"] += 1
                if last:
                    sampler.candidates(logits, spec)
            elif kind == "decode":
                _, ids, pos, slots, bt, ctx, spec, graph, ingraph = msg
                stats["decode_steps"] += 1
                if graph and graphs is not None and ingraph:
                    graphs.launch(ids, pos, slots, bt, ctx, fetch=False)
                    stats["ingraph_steps"] += 1
                    stats["lookahead_steps"] += ids is None
                    continue
                if graph and graphs is not None:
                    logits = graphs.run(ids, pos, slots, bt, ctx)
                else:
                    logits = llm.decode(h2d(ids, dev), h2d(pos, dev), h2d(slots, dev), kv, h2d(bt, dev),
                                        h2d(ctx, dev), workspace=ws)
                sampler.candidates(logits, spec)
    stats["d2h"] = sync.stats["d2h"] + sampler.d2h
    stats["transport"] = sync.transport
    path = os.environ.get("LUMEN_TP_FOLLOWER_STATS")
    if path:
        import json

        with open(f"{path}.rank{llm.tp.rank}", "w") as f:
            json.dump(stats, f)
    sync.close()
    return stats
