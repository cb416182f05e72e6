"""The step channel of a tensor-parallel group: rank 0 (the engine) to the follower ranks."""
from __future__ import annotations

import logging
import os
from typing import Optional

import numpy as np
import torch

log = logging.getLogger("lumen.engine")


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
