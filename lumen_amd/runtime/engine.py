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
from .kv_cache import BLOCK, PagedKVCache
from .spec_decode import Drafter, NgramDrafter, drafter_from_env, spec_tokens_from_env  # noqa: F401

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


class TPSync:
    """Step channel from rank 0 (the engine) to the follower ranks of a TP group.

    Transport:

    * ``bus`` (default when every rank of the group is on this node -- always, for
      :class:`~lumen_amd.parallel.tp.TPServingGroup`): a host shared-memory ring
      (:mod:`lumen_amd.parallel.step_bus`).  A follower's host reads the step straight from shared
      memory -- no collective and no device->host copy per token -- and launches its step while
      the leader launches its own.
    * ``bcast``: ONE broadcast of a 4 KiB prefix of an int32 buffer per step (GPU buffer for RCCL,
      host for gloo), plus a sized remainder for long descriptors; the follower copies the prefix
      to the host to parse it.

    A decode step is an 8-int header (op, batch, table width, top-k, flags, message length)
    followed by the step descriptor -- ids, positions, cache slots, context lengths, block table;
    nothing is pickled.  ``flags``: 1 = replay the captured graph, 2 = token ids come from the
    previous replay's in-graph arg-max (look-ahead step), 4 = the graph's in-graph TP sampler is
    this step's sampler (the follower does nothing after the replay).  Prefill / control messages
    and decode steps whose sampling needs per-row state (temperatures, repetition-penalty token
    sets) travel pickled (bus) or as an object broadcast (bcast).
    ``capacity`` (ints after the header) must hold 4 * batch + batch * table width of the
    largest decode step: :func:`tp_sync_capacity`.
    """

    OBJ, DECODE, OBJ_BIG = 1, 2, 3
    F_GRAPH, F_DEV_IDS, F_INGRAPH = 1, 2, 4

    def __init__(self, group=None, src: int = 0, device: Optional[torch.device] = None, capacity: int = 1 << 15,
                 transport: Optional[str] = None):
        import torch.distributed as dist

        self.group, self.src = group, src
        if device is None:
            be = dist.get_backend(group) if dist.is_initialized() else "gloo"
            device = torch.device("cuda", torch.cuda.current_device()) if be == "nccl" else torch.device("cpu")
        self.device = device
        self.capacity = int(capacity)
        self.buf = torch.zeros(8 + self.capacity, dtype=torch.int32, device=device)
        self.prefix = min(1024, 8 + self.capacity)          # ints per step's first broadcast
        self.stats = {"tensor_steps": 0, "object_steps": 0, "two_part_steps": 0, "d2h": 0}
        self.bus = None
        transport = transport or os.environ.get("LUMEN_TP_STEP_TRANSPORT", "bus")
        if transport == "bus":
            self.bus = self._open_bus()
        self.transport = "bus" if self.bus is not None else "bcast"

    def _open_bus(self):
        """Collective: a shared-memory bus when all ranks share this host and the host library
        has it (every rank agrees, else all fall back to broadcasts)."""
        import socket

        import torch.distributed as dist

        from ..parallel import step_bus

        rank, world = dist.get_rank(self.group), dist.get_world_size(self.group)
        hosts = [None] * world
        dist.all_gather_object(hosts, (socket.gethostname(), step_bus.available()), group=self.group)
        if len({h for h, _ in hosts}) != 1 or not all(ok for _, ok in hosts):
            return None
        slot = max(1 << 18, 4 * (8 + self.capacity) + 64)
        name = [None]
        bus, err = None, None
        if rank == self.src:
            try:
                name[0] = step_bus.StepBus.unique_name()
                bus = step_bus.StepBus(name[0], None, nslots=64, slot_bytes=slot, nreaders=world - 1)
            except Exception as e:  # noqa: BLE001 - agreed fallback below
                name[0], err = None, e
        dist.broadcast_object_list(name, src=self.src, group=self.group)
        if name[0] is not None and rank != self.src:
            try:
                bus = step_bus.StepBus(name[0], rank if rank < self.src else rank - 1)
            except Exception as e:  # noqa: BLE001
                bus, err = None, e
        oks = [None] * world
        dist.all_gather_object(oks, bus is not None, group=self.group)
        if rank == self.src and bus is not None:
            bus.unlink()                       # every rank holds its mapping (or gave up): drop the name
        if not all(oks):
            if bus is not None:
                bus.close()
            log.warning("TP step bus unavailable (%s); stepping over broadcasts", err)
            return None
        return bus

    def _bcast(self, t: torch.Tensor) -> None:
        import torch.distributed as dist

        dist.broadcast(t, src=self.src, group=self.group)

    def send(self, msg) -> None:
        import pickle

        import torch.distributed as dist

        self.stats["object_steps"] += 1
        if self.bus is not None:
            data = pickle.dumps(msg, protocol=pickle.HIGHEST_PROTOCOL)
            head = np.zeros(8, np.int32)
            if 32 + len(data) <= self.bus.slot_bytes:
                head[0] = self.OBJ
                self.bus.publish(head.tobytes() + data)
                return
            head[0] = self.OBJ_BIG
            self.bus.publish(head)
        else:
            self.buf[:8].fill_(0)
            self.buf[0] = self.OBJ
            self._bcast(self.buf[:self.prefix])
        dist.broadcast_object_list([msg], src=self.src, group=self.group)

    def send_decode(self, ids, pos, slots, bt, ctx, spec, graph: bool, ingraph: bool = False) -> None:
        """``ids`` None: the previous replay's in-graph arg-max feeds this step (look-ahead)."""
        B, W = len(pos), bt.shape[1]
        if spec["inv"] is not None or spec["pen"] is not None or 4 * B + B * W > self.capacity:
            self.send(("decode", ids, pos, slots, bt, ctx, spec, graph, ingraph))
            return
        n = 8 + 4 * B + B * W
        flags = (self.F_GRAPH if graph else 0) | (self.F_DEV_IDS if ids is None else 0) | \
            (self.F_INGRAPH if ingraph else 0)
        msg = np.zeros(n, np.int32)
        msg[:8] = [self.DECODE, B, W, spec["k"], flags, n, 0, 0]
        if ids is not None:
            msg[8:8 + B] = np.asarray(ids, np.int64).astype(np.int32)
        msg[8 + B:] = np.concatenate([np.asarray(pos, np.int32), np.asarray(slots, np.int64).astype(np.int32),
                                      np.asarray(ctx, np.int32), np.asarray(bt, np.int32).reshape(-1)])
        self.stats["tensor_steps"] += 1
        if self.bus is not None:
            self.bus.publish(msg)
            return
        self.buf[:n].copy_(torch.from_numpy(msg), non_blocking=self.device.type == "cuda")
        self._bcast(self.buf[:self.prefix])
        if n > self.prefix:
            self._bcast(self.buf[self.prefix:n])
            self.stats["two_part_steps"] += 1

    def _parse_decode(self, p: np.ndarray):
        h = p[:8].tolist()
        B, W, k, flags = h[1], h[2], h[3], h[4]
        p = p[8:8 + 4 * B + B * W]
        ids = None if flags & self.F_DEV_IDS else p[:B].astype(np.int64)
        pos = p[B:2 * B].copy()
        slots = p[2 * B:3 * B].astype(np.int64)
        ctx = p[3 * B:4 * B].copy()
        bt = p[4 * B:].reshape(B, W).copy()
        return ("decode", ids, pos, slots, bt, ctx, {"k": k, "inv": None, "pen": None, "pen_ids": None},
                bool(flags & self.F_GRAPH), bool(flags & self.F_INGRAPH))

    def _recv_obj(self):
        import torch.distributed as dist

        obj = [None]
        dist.broadcast_object_list(obj, src=self.src, group=self.group)
        return obj[0]

    def recv(self):
        if self.bus is not None:
            import pickle

            from ..parallel.step_bus import BusClosed

            while True:
                try:
                    m = self.bus.next(timeout_ms=1000)
                except BusClosed:
                    return ("stop",)
                if m is not None:
                    break
                if not self.bus.writer_alive():
                    return ("stop",)
            op = int(np.frombuffer(m[:4], np.int32)[0])
            if op == self.OBJ:
                return pickle.loads(m[32:])     # written by this group's own leader process
            if op == self.OBJ_BIG:
                return self._recv_obj()
            return self._parse_decode(np.frombuffer(m, np.int32))
        self._bcast(self.buf[:self.prefix])
        p = self.buf[:self.prefix].cpu().numpy()
        self.stats["d2h"] += 1
        if int(p[0]) == self.OBJ:
            return self._recv_obj()
        n = int(p[5])
        if n > self.prefix:
            self._bcast(self.buf[self.prefix:n])
            p = self.buf[:n].cpu().numpy()
            self.stats["d2h"] += 1
        return self._parse_decode(p)

    def close(self) -> None:
        if self.bus is not None:
            self.bus.close()
            self.bus = None


def tp_sync_capacity(max_batch: int, max_position: int) -> int:
    """Descriptor ints of the largest decode step: 4 per row + the block table (64-token blocks)."""
    return max_batch * (4 + -(-max_position // 64))


class SeenSlots:
    """The device sampler's seen-token bitmaps: [max_batch, ceil(V / 32)] int32 (19 KB per row at
    V = 151,936), one row = "slot" per penalised request, allocated on first use.  :class:`DecodeGraphs`
    is one; an engine without graphs that samples verify steps holds a bare one."""

    def __init__(self, llm, max_batch: int):
        self.llm = llm
        self.max_batch = max(max_batch, 1)
        self.seen: Optional[torch.Tensor] = None
        self._free_slots = list(range(self.max_batch - 1, -1, -1))

    def _seen(self) -> torch.Tensor:
        if self.seen is None:
            self.seen = torch.zeros((self.max_batch, lops.seen_words(self.llm.Vl)), dtype=torch.int32,
                                    device=self.llm.embed.device)
        return self.seen

    def take_slot(self) -> Optional[int]:
        """a free row of the seen bitmap (None: all taken); fill it with :meth:`write_slot`"""
        return self._free_slots.pop() if self._free_slots else None

    def free_slot(self, slot: int) -> None:
        self._free_slots.append(slot)

    def write_slot(self, slot: int, tokens: Sequence[int]) -> None:
        """Set row ``slot`` of the bitmap to exactly ``tokens`` (none: zero it), on the current
        stream -- the one the graphs replay on, so it lands after every step launched before."""
        seen = self._seen()
        row = np.zeros(seen.shape[1], np.uint32)
        t = np.asarray([x for x in tokens if 0 <= x < self.llm.Vl], np.int64)
        if len(t):
            np.bitwise_or.at(row, t >> 5, np.uint32(1) << (t & 31).astype(np.uint32))
        seen[slot].copy_(torch.from_numpy(row.view(np.int32)))


class GuideArena:
    """The device side of guided decoding: ``LUMEN_GUIDED_STATES`` rows (default 4096; 19 KB each
    at V = 151,936) of allowed-token bitmaps and of byte transitions in arena-global state ids, the
    CSR of the token bytes (one copy per engine) and one grammar state per running sequence.

    Allocated once, before the first ``guided`` graph is captured, so the pointers the graphs hold
    stay valid.  A guide is uploaded on first use into a free run of rows and stays resident; when
    a new one does not fit, the least recently used guides that no running request refers to are
    evicted.  A guide that cannot fit raises :class:`~lumen_amd.runtime.guided.GuideError`, which
    fails that request only."""

    def __init__(self, llm, max_batch: int, token_bytes: Sequence[bytes], rows: Optional[int] = None):
        from .guided import token_csr

        d = llm.embed.device
        self.V = llm.Vl
        self.rows = int(rows or os.environ.get("LUMEN_GUIDED_STATES", 4096))
        if not 1 <= self.rows <= 32767:
            raise ValueError("LUMEN_GUIDED_STATES: 1 .. 32767 (arena-global state ids are int16)")
        self.words = lops.seen_words(self.V)
        self.allow = torch.zeros((self.rows, self.words), dtype=torch.int32, device=d)
        self.dfa = torch.full((self.rows, 256), -1, dtype=torch.int16, device=d)
        self.token_bytes = token_bytes
        tb = list(token_bytes[:self.V]) + [b""] * max(0, self.V - len(token_bytes))
        off, dat = token_csr(tb)
        self.tok_off = torch.from_numpy(off).to(d)
        self.tok_dat = torch.from_numpy(dat.copy()).to(d)
        self.state = torch.zeros(max(max_batch, 1), dtype=torch.int32, device=d)
        self._free_slots = list(range(max(max_batch, 1) - 1, -1, -1))
        self._res: "dict[int, dict]" = {}      # id(guide) -> {"g", "base", "n", "refs"}, least recently used first

    def take_slot(self) -> Optional[int]:
        return self._free_slots.pop() if self._free_slots else None

    def free_slot(self, slot: int) -> None:
        self._free_slots.append(slot)

    def _gap(self, n: int) -> Optional[int]:
        """first row of a free run of ``n`` rows (first fit), or None"""
        at = 0
        for e in sorted(self._res.values(), key=lambda e: e["base"]):
            if e["base"] - at >= n:
                return at
            at = e["base"] + e["n"]
        return at if self.rows - at >= n else None

    def acquire(self, g) -> int:
        """first arena row of guide ``g``, uploading it if it is not resident; takes a reference"""
        from .guided import GuideError

        e = self._res.pop(id(g), None)
        if e is None:
            n = g.n_states
            if g.token_bytes is not self.token_bytes and list(g.token_bytes) != list(self.token_bytes):
                raise GuideError("the guide was compiled for another vocabulary than this engine's guides")
            if n > self.rows or g.V > self.V:
                raise GuideError(f"a guide of {n} states over {g.V} tokens does not fit the arena "
                                 f"(LUMEN_GUIDED_STATES = {self.rows}, vocabulary {self.V})")
            base = self._gap(n)
            while base is None:
                idle = next((k for k, v in self._res.items() if v["refs"] == 0), None)
                if idle is None:
                    raise GuideError(f"no room for a guide of {n} states: the arena's {self.rows} rows "
                                     "(LUMEN_GUIDED_STATES) are held by the guides of running requests")
                del self._res[idle]
                base = self._gap(n)
            # on the current stream, the one the graphs replay on: after every step launched before
            rows = np.zeros((n, self.words), np.int32)
            rows[:, :g.allow.shape[1]] = g.allow
            self.allow[base:base + n].copy_(torch.from_numpy(rows))
            dfa = np.where(g.dfa >= 0, g.dfa.astype(np.int32) + base, -1).astype(np.int16)
            self.dfa[base:base + n].copy_(torch.from_numpy(dfa))
            e = {"g": g, "base": base, "n": n, "refs": 0}
        e["refs"] += 1
        self._res[id(g)] = e                   # most recently used last
        return e["base"]

    def release(self, g) -> None:
        e = self._res.get(id(g))
        if e is not None and e["refs"] > 0:
            e["refs"] -= 1

    def tensors(self, g_slot: torch.Tensor, g_in: torch.Tensor):
        return lops.GuideTensors(self.allow, self.dfa, self.tok_off, self.tok_dat, g_slot, g_in, self.state)


class DecodeGraphs(SeenSlots):
    """hipGraph-captured decode steps, one graph per (padded batch-size, table-width) bucket.

    A decode step is ~5 kernels per layer (hundreds per token) whose host launch cost
    dominates small-batch decode; replaying a captured graph issues them in one call.
    Inputs live in ONE device buffer per graph (positions, context lengths, block table of
    fixed width, cache slots) filled by ONE H2D copy from a pinned staging buffer; padded
    rows use slot -1 (no cache write) and context 1, and their logits are ignored.

    The graph also holds the greedy sampler: the row top-8 candidates + row lse go to one
    packed result buffer (one D2H per step) and the arg-max token is written straight into the
    batch bucket's token-id buffer, which every graph of that bucket embeds from -- so the NEXT
    step can be launched before the host has read this one (:meth:`launch` with ``ids=None``;
    LLMEngine's look-ahead decode).  Under TP the vocab-parallel merge is captured too: each
    rank's shard top-8 + lse go into its row of a [world, B, 20] fp32 block, ONE all-reduce
    (the IPC one-shot kernel) gives every rank every shard's candidates, and the global top-8,
    the lse of the shard lse's and the arg-max are computed on every rank identically -- so the
    followers never read anything back and look-ahead works under TP.  The last word of the
    result buffer is the IPC all-reduce error flag, copied after the step's last all-reduce:
    the leader sees it in the same D2H as the tokens, before emitting them.  Staging and result
    buffers are double-buffered and fenced by the event of the launch that last used them.

    ``mode="sample"`` graphs (single GPU, captured on first need; the greedy graphs, their step
    buffer and their result buffer are untouched by them) end in the device sampler
    (``sample_rows``, csrc/sampler.hip) instead of the top-8 + arg-max: repetition penalty over a
    per-request bitmap of the tokens fed so far (``seen``, one row = "slot" per penalised
    request), temperature, top-64 candidates, nucleus cut and the draw with a uniform the host
    supplies, so sampled and penalised requests replay and look ahead like greedy ones.  Their step
    buffer also carries per-row 1/T, top_p, penalty, greedy flag, bitmap slot and uniform; their
    result buffer is the tokens plus the error word.  Padded rows are greedy with slot -1.

    ``mode="verify"`` graphs (speculative decoding, single GPU; again with buffers of their own)
    run :meth:`LLM.verify` over T rows per sequence, at most 32 rows in all: the step buffer carries
    token ids, positions and slots of Bp * T rows and context length, live-row count and block
    table of Bp sequences; the result buffer is the arg-max token of every row plus the error
    word.  Padded rows use slot -1; padded sequences context 1 with one live row.

    ``mode="verify_sample"`` graphs are the verify step with the device sampler's verify form
    (``sample_verify_rows``: the draw of every row, then ``verify_accept``) in place of the row
    arg-max, for batches with sampled or penalised requests.  The step buffer also carries the
    sampler's per-sequence rows (as in ``sample`` mode) and one uniform per row; the result buffer is
    the drawn token of every row, the accepted draft tokens of every sequence and the error word.
    Padded sequences are greedy with slot -1 and one live row.

    ``mode="verify_guided"`` graphs are the ``verify_sample`` graphs with the sampler's guided verify
    form, for batches with a guided request (speculative decoding of guided requests): the step
    buffer also carries ``g_in`` of Bp * T rows, the arena-global grammar state in which each row
    draws (-1 for an unguided, dead or padded row).  No state is kept on the device between verify
    steps.  They need :attr:`arena` like the ``guided`` graphs.

    ``mode="guided"`` graphs are the ``sample`` graphs with the sampler's guided form: the step
    buffer also carries per row the sequence's row of the device's grammar states (``g_slot``, -1
    for an unguided or padded row) and the state the host feeds (``g_in``, -1 on a look-ahead step,
    which reads the state the step before it stored).  They need :attr:`arena` (a
    :class:`GuideArena`), set before the first of them is captured.
    """

    BUCKETS = (1, 2, 4, 8, 16, 32, 64, 128)
    K_GREEDY = 8

    def __init__(self, llm, kv: PagedKVCache, max_batch: int, max_blocks: int):
        SeenSlots.__init__(self, llm, max_batch)     # sample / verify_sample modes: the seen-token bitmaps
        self.kv = kv
        self.max_blocks = max_blocks
        self.buckets = [b for b in self.BUCKETS if b <= max(max_batch, 1)] or [1]
        if self.buckets[-1] < max_batch:
            self.buckets.append(max_batch)
        self.graphs: dict[tuple, dict] = {}
        self.ids: dict[int, torch.Tensor] = {}       # batch bucket -> device token ids (shared by its graphs)
        self.pool = None
        self.in_graph_sampler = not llm.tp.enabled or os.environ.get("LUMEN_TP_INGRAPH_SAMPLER", "1") == "1"
        self._stream = None     # the capture stream, private to this instance (see _capture_stream)
        self.arena: Optional[GuideArena] = None      # guided mode: set by the engine before its first capture

    def _bucket(self, B: int) -> int:
        for b in self.buckets:
            if b >= B:
                return b
        raise ValueError(f"batch {B} exceeds graph buckets {self.buckets}")

    def _width(self, w: int) -> int:
        """block-table width bucket: the decode kernel's split count follows the width,
        so short contexts must not pay for the maximum-length table."""
        for b in (8, 32, 128):
            if w <= b and b <= self.max_blocks:
                return b
        return self.max_blocks

    @staticmethod
    def _layout(Bp: int, W: int) -> dict:
        """byte offsets of (slots i64, pos i32, ctx i32, bt i32) in the step buffer"""
        o_pos = 8 * Bp
        o_ctx = o_pos + 4 * Bp
        o_bt = o_ctx + 4 * Bp
        return {"slots": (0, Bp), "pos": (o_pos, Bp), "ctx": (o_ctx, Bp), "bt": (o_bt, Bp * W),
                "bytes": -(-(o_bt + 4 * Bp * W) // 16) * 16}

    @staticmethod
    def _layout_sample(Bp: int, W: int) -> dict:
        """the greedy layout followed by the sampler's rows: (u f64, top_p f64, inv_t f32, penalty
        f32, greedy i32, seen_slot i32); the f64 rows start 16-byte aligned"""
        lay = dict(DecodeGraphs._layout(Bp, W))
        o = lay["bytes"]
        for k, sz in (("u", 8), ("top_p", 8), ("inv_t", 4), ("penalty", 4), ("greedy", 4), ("seen_slot", 4)):
            lay[k] = (o, Bp)
            o += sz * Bp
        lay["bytes"] = -(-o // 16) * 16
        return lay

    _SAMPLE_ROWS = {"u": torch.float64, "top_p": torch.float64, "inv_t": torch.float32, "penalty": torch.float32,
                    "greedy": torch.int32, "seen_slot": torch.int32}
    _SAMPLE_PAD = {"u": 0.0, "top_p": 1.0, "inv_t": 1.0, "penalty": 1.0, "greedy": 1, "seen_slot": -1}
    _GUIDE_ROWS = {"g_slot": torch.int32, "g_in": torch.int32}      # guided mode, after the sampler's rows
    _GUIDE_PAD = {"g_slot": -1, "g_in": -1}

    @staticmethod
    def _layout_guided(Bp: int, W: int) -> dict:
        """the sample layout followed by (g_slot i32, g_in i32)"""
        lay = dict(DecodeGraphs._layout_sample(Bp, W))
        o = lay["bytes"]
        for k in DecodeGraphs._GUIDE_ROWS:
            lay[k] = (o, Bp)
            o += 4 * Bp
        lay["bytes"] = -(-o // 16) * 16
        return lay

    def _capture_stream(self, d: torch.device) -> torch.cuda.Stream:
        """One stream per engine that nothing else ever uses.  The split-K tickets and
        workspaces the kernels key by stream are baked into the graphs captured on it; a
        stream from PyTorch's recycled pool could later be handed to another thread's eager
        split-K work while a graph replays, and the two would share counters."""
        if self._stream is None:
            self._stream = ops.private_stream(d)
        return self._stream

    def _record(self, run, d: torch.device):
        """Warm ``run`` up twice on the private stream, then capture it; returns (graph, run's result)."""
        s = self._capture_stream(d)
        s.wait_stream(torch.cuda.current_stream(d))
        with torch.cuda.stream(s):
            for _ in range(2):
                run()
        torch.cuda.current_stream(d).wait_stream(s)
        g = torch.cuda.CUDAGraph()
        if self.pool is None:
            self.pool = torch.cuda.graph_pool_handle()
        # captured on the warm-up stream: the split-K tickets / workspaces the kernels key by stream
        # already exist (a first request inside the capture would record its zero-fill into every replay)
        # thread_local: a multi-service engine process runs other services' batch loops on other
        # threads meanwhile; the default (global) mode would fail their HIP calls during the capture
        # (ops.CAPTURE_LOCK: one capture at a time in the process, see there)
        with ops.CAPTURE_LOCK, torch.cuda.graph(g, pool=self.pool, stream=s, capture_error_mode="thread_local"):
            out = run()
        return g, out

    def _capture(self, Bp: int, W: int, mode: str = "greedy") -> dict:
        d = self.llm.embed.device
        guided = mode == "guided"
        sample = mode == "sample" or guided
        if guided and self.arena is None:
            raise RuntimeError("guided graphs need the guide arena")
        lay = self._layout_guided(Bp, W) if guided else self._layout_sample(Bp, W) if sample else self._layout(Bp, W)
        dbuf = torch.zeros(lay["bytes"], dtype=torch.uint8, device=d)

        def views(buf):
            o, n = lay["slots"]
            v = {"slots": buf[o:o + 8 * n].view(torch.int64)}
            for k in ("pos", "ctx"):
                o, n = lay[k]
                v[k] = buf[o:o + 4 * n].view(torch.int32)
            o, n = lay["bt"]
            v["bt"] = buf[o:o + 4 * n].view(torch.int32).view(Bp, W)
            if sample:
                for k, dt in self._SAMPLE_ROWS.items():
                    o, n = lay[k]
                    v[k] = buf[o:o + dt.itemsize * n].view(dt)
            if guided:
                for k, dt in self._GUIDE_ROWS.items():
                    o, n = lay[k]
                    v[k] = buf[o:o + dt.itemsize * n].view(dt)
            return v

        st = views(dbuf)
        st["slots"].fill_(-1)
        st["ctx"].fill_(1)
        if sample:
            for k, pad in self._SAMPLE_PAD.items():
                st[k].fill_(pad)
        if guided:
            for k, pad in self._GUIDE_PAD.items():
                st[k].fill_(pad)
            ar = self.arena
        if Bp not in self.ids:
            self.ids[Bp] = torch.zeros(Bp, dtype=torch.long, device=d)
        ids = self.ids[Bp]
        k = self.K_GREEDY
        res = torch.zeros(2 * Bp * k + Bp + 1, dtype=torch.float32, device=d) if self.in_graph_sampler else None
        if sample:
            res = torch.zeros(Bp + 1, dtype=torch.int32, device=d)      # tokens + the error word
            seen = self._seen()
        tp = self.llm.tp
        KP = 2 * k + 4                      # per-row candidate record: k values, k ids, lse, pad to 16 B
        gat = torch.zeros((tp.world, Bp, KP), dtype=torch.float32, device=d) if res is not None and tp.enabled \
            else None
        loc = torch.zeros(2 * Bp * k + Bp, dtype=torch.float32, device=d) if gat is not None else None
        ws: dict = {}

        def run():
            logits = self.llm.decode(ids, st["pos"], st["slots"], self.kv, st["bt"], st["ctx"], workspace=ws)
            if guided:
                # the sample call below with the guided form's tensors: masks by the row's grammar state
                # (st["g_in"], or the arena's state array on a look-ahead step) and stores the new state
                ops.hip_ops().sample_rows(logits, st["inv_t"], st["top_p"], st["penalty"], st["u"], st["greedy"],
                                          st["seen_slot"], seen, ids, ids, res[:Bp], None, None, None,
                                          ar.allow, ar.dfa, ar.tok_off, ar.tok_dat, st["g_slot"], st["g_in"],
                                          ar.state)
            elif sample:
                # reads ids (the step's input tokens: penalised and marked) and writes the drawn ones back
                ops.hip_ops().sample_rows(logits, st["inv_t"], st["top_p"], st["penalty"], st["u"], st["greedy"],
                                          st["seen_slot"], seen, ids, ids, res[:Bp], None, None, None)
            elif res is not None:
                v = res[:Bp * k].view(Bp, k)
                i = res[Bp * k:2 * Bp * k].view(torch.int32).view(Bp, k)
                lse = res[2 * Bp * k:2 * Bp * k + Bp]
                hip = ops.hip_ops()
                if gat is None:
                    hip.row_topk(logits, k, 1.0, v, i, lse, int(self.llm.v0))
                else:
                    lv = loc[:Bp * k].view(Bp, k)
                    li = loc[Bp * k:2 * Bp * k].view(torch.int32).view(Bp, k)
                    hip.row_topk(logits, k, 1.0, lv, li, loc[2 * Bp * k:], int(self.llm.v0))
                    gat.zero_()
                    own = gat[tp.rank]
                    own[:, :k].copy_(lv)
                    own[:, k:2 * k].copy_(li)                 # global vocab ids < 2^24: exact in fp32
                    own[:, 2 * k].copy_(loc[2 * Bp * k:])
                    self.llm._all_reduce(gat)
                    vals = gat[:, :, :k].permute(1, 0, 2).reshape(Bp, tp.world * k)
                    gids = gat[:, :, k:2 * k].permute(1, 0, 2).reshape(Bp, tp.world * k)
                    tv, order = torch.topk(vals, k, dim=1)
                    v.copy_(tv)
                    i.copy_(torch.gather(gids, 1, order))
                    lse.copy_(torch.logsumexp(gat[:, :, 2 * k], 0))
                    comm = getattr(self.llm, "comm", None)
                    if comm is not None:
                        comm.error_into(res[2 * Bp * k + Bp:].view(torch.int32))
                ids.copy_(i[:, 0])                                   # greedy next token, on the device
            return logits

        g, out = self._record(run, d)
        pin = lambda t: torch.empty(t.shape, dtype=t.dtype).pin_memory()  # noqa: E731
        ent = {"g": g, "st": st, "dbuf": dbuf, "out": out, "ws": ws, "res": res, "lay": lay, "Bp": Bp, "W": W,
               "h_step": [pin(dbuf) for _ in range(2)], "h_ids": [pin(ids) for _ in range(2)],
               "h_res": [pin(res) for _ in range(2)] if res is not None else None,
               "ev": [None, None], "par": 0, "mode": mode}
        ent["h_views"] = [views(h) for h in ent["h_step"]]
        self.graphs[(Bp, W, mode)] = ent
        return ent

    def _entry(self, B: int, width: int, mode: str = "greedy") -> dict:
        key = (self._bucket(B), self._width(width), mode)
        return self.graphs[key] if key in self.graphs else self._capture(*key)

    def launch(self, ids, pos, slots, bt, ctx, fetch: bool = True, sample: Optional[dict] = None) -> dict:
        """Stage + replay one step (host arrays; ``ids=None``: the token ids the previous
        replay of this batch bucket wrote on the device).  Returns a handle for
        :meth:`tokens` / :meth:`logits`.  ``fetch=False`` (TP followers): no result copy.
        ``sample``: per-row arrays of the device sampler (keys of ``_SAMPLE_ROWS``) -- the step
        runs the ``sample`` graph and :meth:`sampled` reads its tokens; with the keys of
        ``_GUIDE_ROWS`` too, the ``guided`` graph."""
        B = len(pos)
        guided = sample is not None and "g_slot" in sample
        e = self._entry(B, bt.shape[1], "greedy" if sample is None else "guided" if guided else "sample")
        Bp, W = e["Bp"], e["W"]
        par = e["par"]
        e["par"] ^= 1
        if e["ev"][par] is not None:
            e["ev"][par].synchronize()        # the copies that last used these pinned buffers are done
        hv = e["h_views"][par]
        w = min(bt.shape[1], W)
        sl, po, cx, tb = (hv[k].numpy() for k in ("slots", "pos", "ctx", "bt"))
        sl[:] = -1
        sl[:B] = slots
        po[:] = 0
        po[:B] = pos
        cx[:] = 1
        cx[:B] = ctx
        tb[:] = 0
        tb[:B, :w] = bt[:, :w]
        if sample is not None:
            for k, pad in self._SAMPLE_PAD.items():
                a = hv[k].numpy()
                a[:] = pad
                a[:B] = sample[k]
            if guided:
                for k, pad in self._GUIDE_PAD.items():
                    a = hv[k].numpy()
                    a[:] = pad
                    a[:B] = sample[k]
        e["dbuf"].copy_(e["h_step"][par], non_blocking=True)
        if ids is not None:
            hi = e["h_ids"][par].numpy()
            hi[:] = 0
            hi[:B] = ids
            self.ids[Bp].copy_(e["h_ids"][par], non_blocking=True)
        e["g"].replay()
        if e["res"] is not None and fetch:
            e["h_res"][par].copy_(e["res"], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        e["ev"][par] = ev
        return {"e": e, "par": par, "B": B, "ev": ev}

    def tokens(self, h: dict):
        """(values [B, 8], ids [B, 8], lse [B]) numpy of a launched step (waits for it); sets
        ``h["err"]`` from the step's all-reduce error word (TP)."""
        e, B = h["e"], h["B"]
        h["ev"].synchronize()
        r = e["h_res"][h["par"]]
        Bp, k = e["Bp"], self.K_GREEDY
        h["err"] = int(r[2 * Bp * k + Bp:].view(torch.int32)[0])
        v = r[:Bp * k].view(Bp, k)[:B].numpy()
        i = r[Bp * k:2 * Bp * k].view(torch.int32).view(Bp, k)[:B].numpy()
        return v, i, r[2 * Bp * k:2 * Bp * k + B].numpy()

    def sampled(self, h: dict) -> np.ndarray:
        """tokens [B] int32 of a launched ``sample`` step (waits for it); sets ``h["err"]``"""
        e, B = h["e"], h["B"]
        h["ev"].synchronize()
        r = e["h_res"][h["par"]].numpy()
        h["err"] = int(r[e["Bp"]])
        return r[:B]

    # ---- verify mode (speculative decoding): up to T rows per sequence, single GPU
    def verify_bucket(self, B: int, T: int) -> int:
        """padded sequence count of a verify step: the batch bucket while its rows fit the 32-row
        decode GEMMs, else the largest count that does"""
        Bp = self._bucket(B)
        return Bp if Bp * T <= 32 else 32 // T

    @staticmethod
    def _layout_verify(Bp: int, W: int, T: int) -> dict:
        """byte offsets of (slots i64, ids i64, pos i32: Bp * T rows; ctx, n_rows, bt i32: Bp sequences)"""
        R = Bp * T
        o_ids = 8 * R
        o_pos = o_ids + 8 * R
        o_ctx = o_pos + 4 * R
        o_n = o_ctx + 4 * Bp
        o_bt = o_n + 4 * Bp
        return {"slots": (0, R), "ids": (o_ids, R), "pos": (o_pos, R), "ctx": (o_ctx, Bp), "n_rows": (o_n, Bp),
                "bt": (o_bt, Bp * W), "bytes": -(-(o_bt + 4 * Bp * W) // 16) * 16}

    @staticmethod
    def _layout_verify_sample(Bp: int, W: int, T: int) -> dict:
        """the verify layout followed by the sampler's rows: u f64 of Bp * T rows, then (top_p f64,
        inv_t f32, penalty f32, greedy i32, seen_slot i32) of Bp sequences; the f64 rows start
        16-byte aligned"""
        lay = dict(DecodeGraphs._layout_verify(Bp, W, T))
        o = lay["bytes"]
        for k, sz, n in (("u", 8, Bp * T), ("top_p", 8, Bp), ("inv_t", 4, Bp), ("penalty", 4, Bp), ("greedy", 4, Bp),
                         ("seen_slot", 4, Bp)):
            lay[k] = (o, n)
            o += sz * n
        lay["bytes"] = -(-o // 16) * 16
        return lay

    @staticmethod
    def _layout_verify_guided(Bp: int, W: int, T: int) -> dict:
        """the verify_sample layout followed by g_in i32 of Bp * T rows"""
        lay = dict(DecodeGraphs._layout_verify_sample(Bp, W, T))
        lay["g_in"] = (lay["bytes"], Bp * T)
        lay["bytes"] = -(-(lay["bytes"] + 4 * Bp * T) // 16) * 16
        return lay

    def _capture_verify(self, Bp: int, W: int, T: int, sample: bool = False, guided: bool = False) -> dict:
        """``sample``: the ``verify_sample`` graph -- the device sampler's verify form and its accept
        kernel in place of the row arg-max; ``res`` = tok [Bp * T], n_acc [Bp] and the error word.
        ``guided``: the ``verify_guided`` graph -- the same with the sampler's guided verify form"""
        d = self.llm.embed.device
        sample = sample or guided
        if guided and self.arena is None:
            raise RuntimeError("guided graphs need the guide arena")
        lay = self._layout_verify_guided(Bp, W, T) if guided else self._layout_verify_sample(Bp, W, T) if sample \
            else self._layout_verify(Bp, W, T)
        R, k = Bp * T, self.K_GREEDY
        dbuf = torch.zeros(lay["bytes"], dtype=torch.uint8, device=d)

        def views(buf):
            v = {}
            for name, dt in (("slots", torch.int64), ("ids", torch.int64), ("pos", torch.int32),
                             ("ctx", torch.int32), ("n_rows", torch.int32), ("bt", torch.int32)):
                o, n = lay[name]
                v[name] = buf[o:o + dt.itemsize * n].view(dt)
            v["bt"] = v["bt"].view(Bp, W)
            if sample:
                for name, dt in self._SAMPLE_ROWS.items():
                    o, n = lay[name]
                    v[name] = buf[o:o + dt.itemsize * n].view(dt)
            if guided:
                o, n = lay["g_in"]
                v["g_in"] = buf[o:o + 4 * n].view(torch.int32)
            return v

        st = views(dbuf)
        st["slots"].fill_(-1)
        st["ctx"].fill_(1)
        st["n_rows"].fill_(1)
        ws: dict = {}
        if sample:
            for name, pad in self._SAMPLE_PAD.items():
                st[name].fill_(pad)
            res = torch.zeros(R + Bp + 1, dtype=torch.int32, device=d)
            seen = self._seen()
            gargs = ()
            if guided:
                st["g_in"].fill_(-1)
                ar = self.arena
                # the guided verify form reads the arena's allow rows and g_in; the slot argument is not read
                gargs = (ar.allow, ar.dfa, ar.tok_off, ar.tok_dat, st["g_in"], st["g_in"], ar.state)

            def run():
                logits = self.llm.verify(st["ids"], st["pos"], st["slots"], self.kv, st["bt"], st["ctx"], st["n_rows"],
                                         T, workspace=ws)
                ops.hip_ops().sample_verify_rows(logits, T, st["n_rows"], st["inv_t"], st["top_p"], st["penalty"],
                                                 st["u"], st["greedy"], st["seen_slot"], seen, st["ids"], res[:R],
                                                 res[R:R + Bp], None, None, None, *gargs)
                return logits
        else:
            res = torch.zeros(R + 1, dtype=torch.int32, device=d)          # arg-max token per row + the error word
            cand = torch.zeros(2 * R * k + R, dtype=torch.float32, device=d)

            def run():
                logits = self.llm.verify(st["ids"], st["pos"], st["slots"], self.kv, st["bt"], st["ctx"], st["n_rows"],
                                         T, workspace=ws)
                i = cand[R * k:2 * R * k].view(torch.int32).view(R, k)
                ops.hip_ops().row_topk(logits, k, 1.0, cand[:R * k].view(R, k), i, cand[2 * R * k:], int(self.llm.v0))
                res[:R].copy_(i[:, 0])
                return logits

        g, out = self._record(run, d)
        pin = lambda t: torch.empty(t.shape, dtype=t.dtype).pin_memory()  # noqa: E731
        mode = "verify_guided" if guided else "verify_sample" if sample else "verify"
        ent = {"g": g, "st": st, "dbuf": dbuf, "out": out, "ws": ws, "res": res, "lay": lay, "Bp": Bp, "W": W, "T": T,
               "h_step": [pin(dbuf) for _ in range(2)], "h_res": [pin(res) for _ in range(2)],
               "ev": [None, None], "par": 0, "mode": mode}
        ent["h_views"] = [views(h) for h in ent["h_step"]]
        self.graphs[(Bp, W, mode)] = ent
        return ent

    def _entry_verify(self, B: int, width: int, T: int, sample: bool = False, guided: bool = False) -> dict:
        key = (self.verify_bucket(B, T), self._width(width),
               "verify_guided" if guided else "verify_sample" if sample else "verify")
        e = self.graphs.get(key)
        return e if e is not None and e["T"] == T else self._capture_verify(key[0], key[1], T, sample, guided)

    def launch_verify(self, ids, pos, slots, bt, ctx, n_rows, T: int, sample: Optional[dict] = None) -> dict:
        """Stage + replay one verify step: ids / pos / slots host arrays of B * T rows
        (sequence-major, padding rows slot -1), ctx / n_rows of B sequences.  Returns a handle
        for :meth:`verified`.  ``sample``: the device sampler's arrays (keys of ``_SAMPLE_ROWS``;
        ``u`` of B * T rows, the others of B sequences) -- the step runs the ``verify_sample`` graph;
        with ``g_in`` (B * T rows) too, the ``verify_guided`` graph."""
        B = len(ctx)
        guided = sample is not None and "g_in" in sample
        e = self._entry_verify(B, bt.shape[1], T, sample is not None, guided)
        W = e["W"]
        par = e["par"]
        e["par"] ^= 1
        if e["ev"][par] is not None:
            e["ev"][par].synchronize()        # the copies that last used these pinned buffers are done
        hv = {k: v.numpy() for k, v in e["h_views"][par].items()}
        w = min(bt.shape[1], W)
        for k, pad, val in (("slots", -1, slots), ("ids", 0, ids), ("pos", 0, pos)):
            hv[k][:] = pad
            hv[k][:B * T] = val
        for k, val in (("ctx", ctx), ("n_rows", n_rows)):
            hv[k][:] = 1
            hv[k][:B] = val
        hv["bt"][:] = 0
        hv["bt"][:B, :w] = bt[:, :w]
        if sample is not None:
            for k, pad in self._SAMPLE_PAD.items():
                hv[k][:] = pad
                hv[k][:len(sample[k])] = sample[k]
            if guided:
                hv["g_in"][:] = -1
                hv["g_in"][:B * T] = sample["g_in"]
        e["dbuf"].copy_(e["h_step"][par], non_blocking=True)
        e["g"].replay()
        e["h_res"][par].copy_(e["res"], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        e["ev"][par] = ev
        return {"e": e, "par": par, "B": B, "ev": ev}

    def verified(self, h: dict) -> np.ndarray:
        """tokens [B * T] int32 of a launched verify step -- the arg-max of every row, or what the
        ``verify_sample`` / ``verify_guided`` graph drew (then ``h["n_acc"]`` holds the device's accepted counts [B]) --
        (waits for it); sets ``h["err"]``"""
        e = h["e"]
        h["ev"].synchronize()
        r = e["h_res"][h["par"]].numpy()
        R = e["Bp"] * e["T"]
        if e["mode"] in ("verify_sample", "verify_guided"):
            h["n_acc"] = r[R:R + h["B"]]
            h["err"] = int(r[R + e["Bp"]])
        else:
            h["err"] = int(r[R])
        return r[:h["B"] * e["T"]]

    def run(self, ids, pos, slots, bt, ctx) -> torch.Tensor:
        """Replay one step and return its logits [B, V/tp] (device, valid until the next replay)."""
        h = self.launch(ids, pos, slots, bt, ctx)
        return h["e"]["out"][:h["B"]]


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
        if self._slots is None and ((self.spec_sampling and self.drafter is not None) or self.spec_guided):
            self._slots = SeenSlots(llm, max_batch)
        self._thread = threading.Thread(target=self._loop, name=f"lumen-{name}-engine", daemon=True)
        self._thread.start()

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
               hit: Optional[PrefixHit] = None, prompt_ids: Optional[Sequence[int]] = None) -> GenRequest:
        """``prefix_keys``: uint64 [n, 2], key i covering prompt tokens [64 i, 64 i + 64) and chaining
        key i - 1 -- the prompt may start from cached blocks and publishes its own after prefill.
        ``hit``: the result of an earlier :meth:`match_prefix` with the same keys (the request
        takes over its id and references).  The prefill builder must return all ``prompt_len``
        rows; rows before the hit are never read.
        ``prompt_ids``: the prompt's token ids for the speculative-decoding drafter (without them
        it sees the generated tokens only)."""
        try:
            if self._stop.is_set():
                raise RuntimeError("engine stopped")
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
                       cached_tokens=hit.tokens, prefix_keys=keys, prompt_ids=prompt_ids)
        if params.guide is not None:
            r.gstate = params.guide.start
        self._waiting.put(r)
        return r

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

    @staticmethod
    def _penalised(r: GenRequest) -> bool:
        return abs(float(r.params.repetition_penalty) - 1.0) > 1e-6

    def _join(self, r: GenRequest) -> None:
        """``r`` enters the running batch; a penalised request takes a zeroed row of the device
        sampler's seen bitmap (none free, or no graphs: its batches sample on the host)"""
        wanted = (self.ingraph_sampling and self.graphs is not None) or \
            (((self.spec_sampling and self.drafter is not None) or self.spec_guided) and self._slots is not None)
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
        logits = self.llm.prefill(r.x[s:e], self.kv, h2d_ahead(slots, self.device), start_pos=s,
                                  prefix_blocks=h2d_ahead(tab, self.device) if tab is not None else None)
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
        ps = [r.params for r in reqs]
        out = {"inv_t": np.array([1.0 / p.temperature if p.temperature > 0 else 1.0 for p in ps], np.float32),
               "top_p": np.array([p.top_p for p in ps], np.float64),
               "penalty": np.array([float(p.repetition_penalty) if r.seen_slot is not None else 1.0
                                    for p, r in zip(ps, reqs)], np.float32),
               "greedy": np.array([p.temperature <= 0 for p in ps], np.int32),
               "seen_slot": np.array([-1 if r.seen_slot is None else r.seen_slot for r in reqs], np.int32),
               "u": np.array([self._uniform(r, len(r.tokens) + ahead) for r in reqs], np.float64)}
        if guided:
            # a fed step carries the state the host derived from the request's tokens; a look-ahead
            # step reads the one the step before it stored, so a discarded look-ahead step that is
            # launched again as a fed step cannot advance the state twice
            gd = [r.params.guide is not None for r in reqs]
            out["g_slot"] = np.array([r.guide_slot if g else -1 for r, g in zip(reqs, gd)], np.int32)
            out["g_in"] = np.array([r.guide_base + r.gstate if g and fed else -1 for r, g in zip(reqs, gd)], np.int32)
        return out

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
            self.graphs._entry(len(reqs), w, mode)
            return True
        except Exception as e:  # noqa: BLE001 - capture unsupported: eager launches from now on
            log.warning("hipGraph decode disabled: %s", e)
            self.graphs = None
            return False

    def _step_inputs(self, reqs, ahead: int):
        """positions / slots / block table / context lengths of the step that feeds position
        r.ctx + ahead of every request"""
        pos = np.array([r.ctx + ahead for r in reqs], np.int32)
        slots = np.concatenate([self.kv.slots(r.rid, r.ctx + ahead, 1) for r in reqs])
        bt = self.kv.block_table([r.rid for r in reqs])
        return pos, slots, bt, pos + 1

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
        ps = [r.params for r in reqs]
        return {"inv_t": np.array([1.0 / p.temperature if p.temperature > 0 else 1.0 for p in ps], np.float32),
                "top_p": np.array([p.top_p for p in ps], np.float64),
                "penalty": np.array([float(p.repetition_penalty) if r.seen_slot is not None else 1.0
                                     for p, r in zip(ps, reqs)], np.float32),
                "greedy": np.array([p.temperature <= 0 for p in ps], np.int32),
                "seen_slot": np.array([-1 if r.seen_slot is None else r.seen_slot for r in reqs], np.int32),
                "u": np.array([self._uniform(r, len(r.tokens) + i, len(r.tokens)) for r in reqs for i in range(T)],
                              np.float64)}

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
            pos[o:o + n] = r.ctx + np.arange(n)
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
            except Exception as e:  # noqa: BLE001 - capture unsupported: eager launches from now on
                log.warning("hipGraph decode disabled: %s", e)
                self.graphs = None
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
        still = []
        for b, (r, d) in enumerate(zip(reqs, drafts)):
            row, j = am[b * T:b * T + 1 + len(d)], acc[b]
            if smp:
                r.seen_n = len(r.tokens) + j      # the accept kernel marked tokens[-1] and the accepted draft tokens
            self.stats["spec_drafted"] += len(d)
            self.stats["spec_accepted"] += j
            if r.draft_forced:
                self.stats["spec_forced_drafted"] += len(d)
                self.stats["spec_forced_accepted"] += j
            done = False
            for t in row[:j + 1]:
                r.ctx += 1
                if self._emit(r, int(t)):
                    done = True
                    break
            if done:
                self._finish(r)
            else:
                still.append(r)
        self._running = still

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
            still = []
            for r, t in zip(reqs, toks):
                r.ctx += 1
                if self._emit(r, t):
                    self._finish(r)
                else:
                    still.append(r)
            self._running = still
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
        pos = np.array([r.ctx for r in reqs], np.int32)
        slots = np.concatenate([self.kv.slots(r.rid, r.ctx, 1) for r in reqs])
        bt = self.kv.block_table([r.rid for r in reqs])
        ctx = pos + 1
        graph = self.graphs is not None and bt.shape[1] <= self.graphs.max_blocks
        if self.sync is not None:
            self.sync.send_decode(ids, pos, slots, bt, ctx, spec, graph)
        logits = self._decode_step(ids, pos, slots, bt, ctx, graph)
        toks = self.sampler.pick(self.sampler.candidates(logits, spec), reqs, self._uniform)
        self.stats["decode_steps"] += 1
        comm = getattr(self.llm, "comm", None)
        if comm is not None:
            comm.check()    # before emitting; the tokens' D2H already waited for the step
        still = []
        for r, t in zip(reqs, toks):
            r.ctx += 1
            if self._emit(r, t):
                self._finish(r)
            else:
                still.append(r)
        self._running = still

    def _launch_greedy(self, ids, inputs, spec, sample: Optional[dict] = None) -> dict:
        """One in-graph-sampled step (``ids`` None: look-ahead, ids from the device); under TP the
        followers get the descriptor first and replay the same graph.  ``sample``: the device
        sampler's per-row inputs (single GPU) instead of the greedy arg-max."""
        if self.sync is not None:
            self.sync.send_decode(ids, *inputs, spec, graph=True, ingraph=True)
        try:
            return self.graphs.launch(ids, *inputs, sample=sample)
        except Exception:
            if self.sync is not None:
                raise            # TP ranks must not diverge
            log.warning("hipGraph decode disabled", exc_info=True)
            self.graphs = None
            raise

    def _decode_step(self, ids, pos, slots, bt, ctx, graph: bool = True) -> torch.Tensor:
        d = self.device
        if graph and self.graphs is not None and bt.shape[1] <= self.graphs.max_blocks:
            try:
                return self.graphs.run(ids, pos, slots, bt, ctx)
            except Exception as e:  # noqa: BLE001 - capture unsupported: fall back to eager launches
                if self.sync is not None:
                    raise            # TP ranks must not diverge: surface instead of falling back
                log.warning("hipGraph decode disabled: %s", e)
                self.graphs = None
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
