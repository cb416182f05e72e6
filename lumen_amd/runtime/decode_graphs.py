"""hipGraph-captured decode and verify steps (:class:`DecodeGraphs`) and the device state they share
(:class:`SeenSlots`, :class:`GuideArena`).

Every graph reads its inputs from one byte buffer, the step buffer, filled by one H2D copy.  Its
contents are described once, by the table below -- fields (name, dtype, extent, pad), groups of
fields, modes as lists of groups -- and :func:`step_layout`, :func:`step_views`, :func:`pad_fill`
and :func:`stage` derive offsets, typed views, the padding at capture and the per-step staging from
it for every mode alike.  They work on any ``uint8`` tensor, so they are tested without a GPU."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, Optional, Sequence

import numpy as np
import torch

from .. import ops
from ..ops import llm as lops
from .kv_cache import PagedKVCache


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

    def args(self, g_slot: torch.Tensor, g_in: torch.Tensor) -> tuple:
        """the seven guide arguments of the device sampler's calls, for these rows' slots and states"""
        return (self.allow, self.dfa, self.tok_off, self.tok_dat, g_slot, g_in, self.state)

    def tensors(self, g_slot: torch.Tensor, g_in: torch.Tensor):
        return lops.GuideTensors(*self.args(g_slot, g_in))


# ---- the step buffer: one table for all modes
ROW, SEQ, TABLE = "row", "seq", "table"      # a field's extent: Bp * T rows, Bp sequences, the [Bp, W] block table


@dataclass(frozen=True)
class Field:
    name: str
    dtype: torch.dtype
    extent: str
    pad: Any            # what padded rows / sequences hold: no cache write, context 1, one live row, greedy, unguided


_SLOTS = Field("slots", torch.int64, ROW, -1)
_IDS = Field("ids", torch.int64, ROW, 0)
_POS = Field("pos", torch.int32, ROW, 0)
_CTX = Field("ctx", torch.int32, SEQ, 1)
_N_ROWS = Field("n_rows", torch.int32, SEQ, 1)
_BT = Field("bt", torch.int32, TABLE, 0)
_G_IN = Field("g_in", torch.int32, ROW, -1)

# a group is packed tight and its end rounded up to 16 bytes (so the f64 fields start aligned)
DECODE_BASE = (_SLOTS, _POS, _CTX, _BT)
VERIFY_BASE = (_SLOTS, _IDS, _POS, _CTX, _N_ROWS, _BT)
SAMPLER = (Field("u", torch.float64, ROW, 0.0), Field("top_p", torch.float64, SEQ, 1.0),
           Field("inv_t", torch.float32, SEQ, 1.0), Field("penalty", torch.float32, SEQ, 1.0),
           Field("greedy", torch.int32, SEQ, 1), Field("seen_slot", torch.int32, SEQ, -1))
GUIDE_DECODE = (Field("g_slot", torch.int32, SEQ, -1), _G_IN)
GUIDE_VERIFY = (_G_IN,)

MODES = {"greedy": (DECODE_BASE,),
         "sample": (DECODE_BASE, SAMPLER),
         "guided": (DECODE_BASE, SAMPLER, GUIDE_DECODE),
         "verify": (VERIFY_BASE,),
         "verify_sample": (VERIFY_BASE, SAMPLER),
         "verify_guided": (VERIFY_BASE, SAMPLER, GUIDE_VERIFY)}
FIELDS = {mode: tuple(f for group in groups for f in group) for mode, groups in MODES.items()}


def is_verify(mode: str) -> bool:
    """the mode's forward is :meth:`LLM.verify` over the step buffer's own token ids"""
    return MODES[mode][0] is VERIFY_BASE


def step_layout(mode: str, Bp: int, W: int, T: int = 1) -> tuple:
    """({field name: (byte offset, entries)}, total bytes) of the mode's step buffer"""
    n = {ROW: Bp * T, SEQ: Bp, TABLE: Bp * W}
    lay, o = {}, 0
    for group in MODES[mode]:
        for f in group:
            lay[f.name] = (o, n[f.extent])
            o += f.dtype.itemsize * n[f.extent]
        o = -(-o // 16) * 16
    return lay, o


def step_views(buf: torch.Tensor, mode: str, Bp: int, W: int, T: int = 1, numpy: bool = False) -> dict:
    """{field name: typed view} over ``buf``, a uint8 tensor of the layout's size on any device
    (the block table as [Bp, W]); ``numpy``: as arrays, for a host buffer that is staged into"""
    lay, size = step_layout(mode, Bp, W, T)
    if buf.dtype != torch.uint8 or buf.numel() != size:
        raise ValueError(f"the {mode} step buffer of ({Bp}, {W}, {T}) is {size} uint8, not {buf.numel()} {buf.dtype}")
    v = {}
    for f in FIELDS[mode]:
        o, n = lay[f.name]
        t = buf[o:o + f.dtype.itemsize * n].view(f.dtype)
        t = t.view(Bp, W) if f.extent is TABLE else t
        v[f.name] = t.numpy() if numpy else t
    return v


def pad_fill(views: dict, mode: str) -> None:
    """every field of the mode holds its pad (tensor views: the device buffer at capture)"""
    for f in FIELDS[mode]:
        views[f.name].fill_(f.pad)


def _put(a: np.ndarray, f: Field, val) -> None:
    """the pad over the whole field, then ``val`` over its leading entries; of a block table the
    columns that fit (a wider one is cut, a narrower one leaves the pad)"""
    a[...] = f.pad
    if f.extent is TABLE:
        w = min(val.shape[1], a.shape[1])
        a[:len(val), :w] = val[:, :w]
    else:
        a[:len(val)] = val


def stage(views: dict, mode: str, values: dict) -> None:
    """Write one step into the numpy views of a host buffer: every field of the mode is padded and
    then takes the caller's values, so nothing of an earlier, larger step survives.  A field the
    caller did not give is an error, never a silent pad."""
    for f in FIELDS[mode]:
        if f.name not in values:
            raise KeyError(f"the {mode} step buffer has a field {f.name!r} that the step does not supply")
        _put(views[f.name], f, values[f.name])


@dataclass
class StepGraph:
    """One captured graph and its buffers.  The pinned host buffers come in pairs, used in turn and
    fenced by the event of the launch that last used them."""
    mode: str
    Bp: int
    W: int
    T: int
    g: Any                          # the graph
    dbuf: torch.Tensor              # the device step buffer ...
    st: dict                        # ... and its typed views, which the captured kernels read
    out: torch.Tensor               # the forward's logits
    ws: dict                        # the forward's workspaces
    res: Optional[torch.Tensor]     # the tail's result buffer
    h_step: list                    # pinned copies of dbuf ...
    h_views: list                   # ... and their numpy views
    h_ids: Optional[list]           # decode modes: pinned token ids for the bucket's shared id buffer
    h_res: Optional[list]
    ev: list
    par: int = 0


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

    A graph has a mode, a key of :data:`MODES`, which says what its step buffer carries; every mode's
    graphs have step and result buffers of their own and are captured on first need.  The decode
    modes run :meth:`LLM.decode` over the bucket's shared token ids and write the next ids back,
    the verify modes (speculative decoding, single GPU) run :meth:`LLM.verify` over T rows per
    sequence, at most 32 rows in all, whose token ids the step buffer carries.  What follows the
    forward, and the result buffer (tokens ... and the error word), differ:

    * ``greedy``: the top-8 + arg-max above, an fp32 buffer with int32 views.
    * ``sample`` (single GPU): the device sampler (``sample_rows``, csrc/sampler.hip): repetition
      penalty over a per-request bitmap of the tokens fed so far (``seen``, one row = "slot" per
      penalised request), temperature, top-64 candidates, nucleus cut and the draw with a uniform
      the host supplies, so sampled and penalised requests replay and look ahead like greedy ones.
      Result: the token of every row.
    * ``guided``: ``sample`` with the sampler's guided form.  ``g_slot`` is the sequence's row of the
      device's grammar states (-1: unguided), ``g_in`` the state the host feeds (-1 on a look-ahead
      step, which reads the state the step before it stored).  Needs :attr:`arena` (a
      :class:`GuideArena`), set before the first capture.
    * ``verify``: the arg-max of every row.
    * ``verify_sample``: the sampler's verify form (``sample_verify_rows``: the draw of every row with
      the row's uniform, then ``verify_accept``), for batches with sampled or penalised requests.
      Result: the drawn token of every row, then the accepted draft tokens of every sequence.
    * ``verify_guided``: ``verify_sample`` with the sampler's guided verify form.  ``g_in`` is the
      arena-global grammar state in which each row draws (-1: unguided or dead row); no state is
      kept on the device between verify steps.  Needs :attr:`arena`.
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
        self.graphs: dict[tuple, StepGraph] = {}      # (Bp, W, mode) -> its graph
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

    def _greedy_tail(self, ids: torch.Tensor, Bp: int):
        """(result buffer, tail) of the greedy graphs: row top-8 + lse into the result buffer -- under TP
        after the captured merge of the shards' candidates, and with the all-reduce error word -- and
        the arg-max into ``ids``.  Without the in-graph sampler (TP switch) there is neither."""
        if not self.in_graph_sampler:
            return None, lambda logits: None
        d, k, tp = ids.device, self.K_GREEDY, self.llm.tp
        res = torch.zeros(2 * Bp * k + Bp + 1, dtype=torch.float32, device=d)
        v = res[:Bp * k].view(Bp, k)
        i = res[Bp * k:2 * Bp * k].view(torch.int32).view(Bp, k)
        lse = res[2 * Bp * k:2 * Bp * k + Bp]
        KP = 2 * k + 4                      # per-row candidate record: k values, k ids, lse, pad to 16 B
        gat = torch.zeros((tp.world, Bp, KP), dtype=torch.float32, device=d) if tp.enabled else None
        loc = torch.zeros(2 * Bp * k + Bp, dtype=torch.float32, device=d) if tp.enabled else None

        def tail(logits):
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
        return res, tail

    def _tail(self, mode: str, st: dict, ids: Optional[torch.Tensor], Bp: int, T: int):
        """(int32 result buffer, tail) of every other mode; the last word is the error word"""
        d, R, hip = st["pos"].device, Bp * T, ops.hip_ops
        if mode == "verify":
            k = self.K_GREEDY
            res = torch.zeros(R + 1, dtype=torch.int32, device=d)
            cand = torch.zeros(2 * R * k + R, dtype=torch.float32, device=d)
            i = cand[R * k:2 * R * k].view(torch.int32).view(R, k)

            def tail(logits):
                hip().row_topk(logits, k, 1.0, cand[:R * k].view(R, k), i, cand[2 * R * k:], int(self.llm.v0))
                res[:R].copy_(i[:, 0])
            return res, tail
        rows = (st["inv_t"], st["top_p"], st["penalty"], st["u"], st["greedy"], st["seen_slot"], self._seen())
        gargs = ()
        if mode in ("guided", "verify_guided"):
            if self.arena is None:
                raise RuntimeError("guided graphs need the guide arena")
            # the verify form reads the arena's allow rows and g_in; its slot argument is not read
            gargs = self.arena.args(st.get("g_slot", st["g_in"]), st["g_in"])
        if ids is not None:
            res = torch.zeros(Bp + 1, dtype=torch.int32, device=d)
            # reads ids (the step's input tokens: penalised and marked) and writes the drawn ones back;
            # guided: masks by the row's grammar state (g_in, or the arena's on a look-ahead step) and stores the new one
            return res, lambda logits: hip().sample_rows(logits, *rows, ids, ids, res[:Bp], None, None, None, *gargs)
        res = torch.zeros(R + Bp + 1, dtype=torch.int32, device=d)
        return res, lambda logits: hip().sample_verify_rows(logits, T, st["n_rows"], *rows, st["ids"], res[:R],
                                                            res[R:R + Bp], None, None, None, *gargs)

    def _capture(self, Bp: int, W: int, mode: str, T: int = 1) -> StepGraph:
        d = self.llm.embed.device
        dbuf = torch.zeros(step_layout(mode, Bp, W, T)[1], dtype=torch.uint8, device=d)
        st = step_views(dbuf, mode, Bp, W, T)
        pad_fill(st, mode)
        ws: dict = {}
        ids = None
        if is_verify(mode):
            def forward():
                return self.llm.verify(st["ids"], st["pos"], st["slots"], self.kv, st["bt"], st["ctx"], st["n_rows"],
                                       T, workspace=ws)
        else:
            if Bp not in self.ids:
                self.ids[Bp] = torch.zeros(Bp, dtype=torch.long, device=d)
            ids = self.ids[Bp]

            def forward():
                return self.llm.decode(ids, st["pos"], st["slots"], self.kv, st["bt"], st["ctx"], workspace=ws)
        res, tail = self._greedy_tail(ids, Bp) if mode == "greedy" else self._tail(mode, st, ids, Bp, T)

        def run():
            logits = forward()
            tail(logits)
            return logits

        g, out = self._record(run, d)
        pin = lambda t: [torch.empty(t.shape, dtype=t.dtype).pin_memory() for _ in range(2)]  # noqa: E731
        h_step = pin(dbuf)
        ent = StepGraph(mode, Bp, W, T, g, dbuf, st, out, ws, res, h_step=h_step,
                        h_views=[step_views(h, mode, Bp, W, T, numpy=True) for h in h_step],
                        h_ids=pin(ids) if ids is not None else None, h_res=pin(res) if res is not None else None,
                        ev=[None, None])
        self.graphs[(Bp, W, mode)] = ent
        return ent

    def ensure(self, B: int, width: int, mode: str = "greedy", T: int = 1) -> StepGraph:
        """the graph that serves a step of ``B`` sequences with a block table ``width`` wide, captured
        if need be -- also when the verify graph of this key was captured for another ``T``"""
        key = (self.verify_bucket(B, T) if is_verify(mode) else self._bucket(B), self._width(width), mode)
        e = self.graphs.get(key)
        return e if e is not None and e.T == T else self._capture(*key, T)

    def _replay(self, e: StepGraph, fields: dict, ids=None, fetch: bool = True) -> dict:
        """Stage ``fields`` (host arrays by field name) and replay ``e``; ``ids``: token ids for the
        bucket's shared id buffer (decode modes; None leaves what the previous replay wrote)."""
        par = e.par
        e.par ^= 1
        if e.ev[par] is not None:
            e.ev[par].synchronize()           # the copies that last used these pinned buffers are done
        stage(e.h_views[par], e.mode, fields)
        e.dbuf.copy_(e.h_step[par], non_blocking=True)
        if ids is not None:
            _put(e.h_ids[par].numpy(), _IDS, ids)
            self.ids[e.Bp].copy_(e.h_ids[par], non_blocking=True)
        e.g.replay()
        if e.res is not None and fetch:
            e.h_res[par].copy_(e.res, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        e.ev[par] = ev
        return {"e": e, "par": par, "B": len(fields["ctx"]), "ev": ev}

    def launch(self, ids, pos, slots, bt, ctx, fetch: bool = True, sample: Optional[dict] = None) -> dict:
        """Stage + replay one step (host arrays; ``ids=None``: the token ids the previous
        replay of this batch bucket wrote on the device).  Returns a handle for
        :meth:`tokens` / :meth:`sampled`.  ``fetch=False`` (TP followers): no result copy.
        ``sample``: the :data:`SAMPLER` fields' per-row arrays -- the step runs the ``sample`` graph
        and :meth:`sampled` reads its tokens; with the :data:`GUIDE_DECODE` fields too, the ``guided`` graph."""
        mode = "greedy" if sample is None else "guided" if "g_slot" in sample else "sample"
        e = self.ensure(len(pos), bt.shape[1], mode)
        return self._replay(e, dict(sample or (), pos=pos, slots=slots, bt=bt, ctx=ctx), ids, fetch)

    def launch_verify(self, ids, pos, slots, bt, ctx, n_rows, T: int, sample: Optional[dict] = None) -> dict:
        """Stage + replay one verify step: ids / pos / slots host arrays of B * T rows
        (sequence-major, padding rows slot -1), ctx / n_rows of B sequences.  Returns a handle
        for :meth:`verified`.  ``sample``: the :data:`SAMPLER` fields' arrays (``u`` of B * T rows, the
        others of B sequences) -- the step runs the ``verify_sample`` graph; with ``g_in`` (B * T rows)
        too, the ``verify_guided`` graph."""
        mode = "verify" if sample is None else "verify_guided" if "g_in" in sample else "verify_sample"
        e = self.ensure(len(ctx), bt.shape[1], mode, T)
        return self._replay(e, dict(sample or (), ids=ids, pos=pos, slots=slots, bt=bt, ctx=ctx, n_rows=n_rows))

    def tokens(self, h: dict):
        """(values [B, 8], ids [B, 8], lse [B]) numpy of a launched step (waits for it); sets
        ``h["err"]`` from the step's all-reduce error word (TP)."""
        e, B = h["e"], h["B"]
        h["ev"].synchronize()
        r = e.h_res[h["par"]]
        Bp, k = e.Bp, self.K_GREEDY
        h["err"] = int(r[2 * Bp * k + Bp:].view(torch.int32)[0])
        v = r[:Bp * k].view(Bp, k)[:B].numpy()
        i = r[Bp * k:2 * Bp * k].view(torch.int32).view(Bp, k)[:B].numpy()
        return v, i, r[2 * Bp * k:2 * Bp * k + B].numpy()

    def sampled(self, h: dict) -> np.ndarray:
        """tokens [B] int32 of a launched ``sample`` step (waits for it); sets ``h["err"]``"""
        e, B = h["e"], h["B"]
        h["ev"].synchronize()
        r = e.h_res[h["par"]].numpy()
        h["err"] = int(r[e.Bp])
        return r[:B]

    # ---- verify mode (speculative decoding): up to T rows per sequence, single GPU
    def verify_bucket(self, B: int, T: int) -> int:
        """padded sequence count of a verify step: the batch bucket while its rows fit the 32-row
        decode GEMMs, else the largest count that does"""
        Bp = self._bucket(B)
        return Bp if Bp * T <= 32 else 32 // T

    def verified(self, h: dict) -> np.ndarray:
        """tokens [B * T] int32 of a launched verify step -- the arg-max of every row, or what the
        ``verify_sample`` / ``verify_guided`` graph drew (then ``h["n_acc"]`` holds the device's accepted counts [B]) --
        (waits for it); sets ``h["err"]``"""
        e = h["e"]
        h["ev"].synchronize()
        r = e.h_res[h["par"]].numpy()
        R = e.Bp * e.T
        if e.mode != "verify":                # the sampler's tails: the accepted counts follow the tokens
            h["n_acc"] = r[R:R + h["B"]]
        h["err"] = int(r[-1])
        return r[:h["B"] * e.T]

    def run(self, ids, pos, slots, bt, ctx) -> torch.Tensor:
        """Replay one step and return its logits [B, V/tp] (device, valid until the next replay)."""
        h = self.launch(ids, pos, slots, bt, ctx)
        return h["e"].out[:h["B"]]

