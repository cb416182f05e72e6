"""Decoder-LLM ops: RoPE tables, fused RoPE + paged KV write, paged decode / prefill / verify
attention, repetition penalty, candidate sampling, the device vocab sampler.

GPU tensors run the HIP kernels of csrc/llm.hip; CPU tensors run fp32 references with
the same semantics (cache layouts in csrc/llm.h: k [NB, Hkv, 64, D], v [NB, Hkv, D, 64]).
"""
from __future__ import annotations

import functools
import math
import os
from typing import Any, NamedTuple, Optional, Sequence

import numpy as np
import torch

from .._native import hip_ops
from ..utils.h2d import h2d
from .moe import moe_experts, moe_grouped_linear, moe_mlp, moe_route, route_weights  # noqa: F401  (the sparse MLP, csrc/moe.hip)

KV_BLOCK = 64


def rope_cos_sin(max_pos: int, head_dim: int, theta: float = 10000.0, scaling: Optional[dict] = None) -> torch.Tensor:
    """[max_pos, D/2, 2] fp32 (cos, sin) with HF inv_freq (+ Llama-3 frequency scaling)."""
    half = head_dim // 2
    inv = 1.0 / (theta ** (torch.arange(0, half, dtype=torch.float64) * 2 / head_dim))
    if scaling and scaling.get("rope_type", scaling.get("type")) == "llama3":
        f = float(scaling.get("factor", 8.0))
        lo, hi = float(scaling.get("low_freq_factor", 1.0)), float(scaling.get("high_freq_factor", 4.0))
        old = float(scaling.get("original_max_position_embeddings", 8192))
        wl = 2 * math.pi / inv
        smooth = (old / wl - lo) / (hi - lo)
        scaled = torch.where(wl > old / lo, inv / f, inv)
        mid = (wl <= old / lo) & (wl >= old / hi)
        scaled = torch.where(mid, (1 - smooth) * inv / f + smooth * inv, scaled)
        inv = scaled
    elif scaling and scaling.get("rope_type", scaling.get("type")) == "linear":
        inv = inv / float(scaling.get("factor", 1.0))
    ang = torch.arange(max_pos, dtype=torch.float64)[:, None] * inv[None, :]
    return torch.stack([torch.cos(ang), torch.sin(ang)], -1).float().contiguous()


def _rot_ref(x: torch.Tensor, cs: torch.Tensor) -> torch.Tensor:
    """x [T, n, D] fp32, cs [T, D/2, 2] -> rotate-half RoPE."""
    half = x.shape[-1] // 2
    c, s = cs[..., 0][:, None, :], cs[..., 1][:, None, :]
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def _qk_norm_ref(x: torch.Tensor, H: int, qk_norm: tuple) -> torch.Tensor:
    """x [T, H + Hkv, D] fp32 -> per-head RMSNorm over D: q heads with q_gamma, k heads with k_gamma."""
    q_gamma, k_gamma, eps = qk_norm
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + float(eps))
    gamma = torch.cat([q_gamma.float().expand(H, -1), k_gamma.float().expand(x.shape[1] - H, -1)], 0)
    return x * rstd * gamma[None]


def _qk_norm_args(op, qk_norm: Optional[tuple]) -> tuple:
    """Trailing (q_gamma, k_gamma, eps) arguments of a HIP op; a library built without them is an error."""
    if qk_norm is None:
        return ()
    if not any(a.name == "q_gamma" for a in op.default._schema.arguments):
        raise RuntimeError(f"{op.default._schema.name}: the native HIP library was built without the per-head "
                           "q / k RMSNorm arguments; rebuild it (python -m lumen_amd._build)")
    q_gamma, k_gamma, eps = qk_norm
    return q_gamma, k_gamma, float(eps)


def mrope_axes(head_dim: int, sections: Sequence[int], interleaved: bool = False) -> torch.Tensor:
    """Multimodal RoPE (Qwen-VL): the position axis of every rotary frequency, uint8 [head_dim / 2]
    with 0 = temporal, 1 = height, 2 = width.  ``sections = [s_t, s_h, s_w]`` sums to head_dim / 2.
    Contiguous layout (Qwen2-VL, Qwen2.5-VL): the first s_t frequencies are temporal, the next s_h
    height, the rest width.  Interleaved (Qwen3-VL): frequency i is height when i % 3 == 1 and
    i < 3 s_h, width when i % 3 == 2 and i < 3 s_w, temporal otherwise."""
    return _mrope_axes(int(head_dim), tuple(int(s) for s in sections), bool(interleaved)).clone()


@functools.lru_cache(maxsize=16)
def _mrope_axes(head_dim: int, sec: tuple, interleaved: bool) -> torch.Tensor:
    """:func:`mrope_axes`, one shared tensor per layout (a prefill asks once per layer): read-only."""
    half = head_dim // 2
    if len(sec) != 3:
        raise ValueError(f"mrope: three sections (temporal, height, width), got {list(sec)}")
    if min(sec) < 0 or sum(sec) != half:
        raise ValueError(f"mrope: sections {list(sec)} must sum to head_dim / 2 = {half}")
    i = torch.arange(half)
    if interleaved:
        ax = torch.where((i % 3 == 1) & (i < 3 * sec[1]), 1, torch.where((i % 3 == 2) & (i < 3 * sec[2]), 2, 0))
    else:
        ax = (i >= sec[0]).long() + (i >= sec[0] + sec[1]).long()
    return ax.to(torch.uint8)


def mrope_positions(ids: Sequence[int], image_token_id: int, grid_hw: tuple) -> tuple[torch.Tensor, int]:
    """Multimodal RoPE positions of a prompt (HF ``get_rope_index``, images only) -> (int32 [3, T], delta).

    ``ids`` are the *expanded* ids: every run of gh * gw ``image_token_id`` is one image whose tokens
    form a gh x gw grid, row-major (``grid_hw = (gh, gw)``).  A text token has t = h = w = n, one more
    than the largest position so far; an image starting at n has t = n, h = n + row, w = n + col and the
    token after it starts at n + max(gh, gw).  ``delta = max(pos) + 1 - T`` (<= 0): generated token at
    cache index c is a text token at position c + delta."""
    gh, gw = int(grid_hw[0]), int(grid_hw[1])
    N = gh * gw
    a = np.asarray(ids, dtype=np.int64).reshape(-1)
    T = a.shape[0]
    pos = np.empty((3, T), np.int32)
    n = i = 0
    while i < T:
        if N > 0 and a[i] == image_token_id and i + N <= T and (a[i:i + N] == image_token_id).all():
            cell = np.arange(N)
            pos[0, i:i + N] = n
            pos[1, i:i + N] = n + cell // gw
            pos[2, i:i + N] = n + cell % gw
            n += max(gh, gw)
            i += N
        else:
            pos[:, i] = n
            n += 1
            i += 1
    return torch.from_numpy(pos), n - T


def _mrope_args(op, axes: Optional[torch.Tensor], qk_norm: Optional[tuple]) -> tuple:
    """Trailing arguments of the HIP rope_kv up to ``mrope_axes``; a library built without it is an error."""
    if axes is None:
        return _qk_norm_args(op, qk_norm)
    if not any(a.name == "mrope_axes" for a in op.default._schema.arguments):
        raise RuntimeError(f"{op.default._schema.name}: the native HIP library was built without the multimodal "
                           "RoPE argument; rebuild it (python -m lumen_amd._build)")
    return (*(_qk_norm_args(op, qk_norm) or (None, None, 0.0)), axes)


def rope_kv(qkv: torch.Tensor, pos: torch.Tensor, cos_sin: torch.Tensor, H: int, Hkv: int, D: int,
            slots: Optional[torch.Tensor] = None, k_cache: Optional[torch.Tensor] = None,
            v_cache: Optional[torch.Tensor] = None, qk_norm: Optional[tuple] = None,
            mrope: Optional[tuple] = None) -> None:
    """Rotate q and k heads of qkv [T, (H + 2Hkv) D] in place; with ``slots`` also write k / v
    of every token into the paged cache (slot = block * 64 + offset, < 0 skipped).

    ``qk_norm = (q_gamma [D], k_gamma [D], eps)`` (fp32, Qwen3): every q / k head vector passes
    through an RMSNorm over D before the rotation, in fp32, rounded once after the rotation;
    v is untouched.  Head dims 32 / 64 / 128 on the GPU.

    ``mrope = (sections, interleaved)`` (Qwen-VL prefill): ``pos`` is [3, T] (temporal, height,
    width) and rotary frequency i takes its angle from the axis :func:`mrope_axes` gives it.  Without
    it ``pos`` is [T]."""
    T = qkv.shape[0]
    axes = None
    if mrope is not None:
        axes = _mrope_axes(int(D), tuple(int(s) for s in mrope[0]), bool(mrope[1]))   # raises on bad sections
        if tuple(pos.shape) != (3, T):
            raise ValueError(f"rope_kv: mrope needs pos [3, {T}], got {list(pos.shape)}")
    elif pos.numel() != T:
        raise ValueError(f"rope_kv: pos [{T}] expected, got {list(pos.shape)} (a [3, T] pos needs mrope)")
    if qkv.is_cuda:
        op = hip_ops().rope_kv
        op(qkv, pos.to(torch.int32).contiguous(), cos_sin,
           slots.to(torch.long).contiguous() if slots is not None else None,
           k_cache if k_cache is not None else qkv, v_cache if v_cache is not None else qkv,
           int(H), int(Hkv), int(D), *_mrope_args(op, axes, qk_norm))
        return
    if T == 0:
        return
    if mrope is not None:
        # frequency i of token t: row pos[axes[i], t] of the table
        cs = cos_sin[pos.long()[axes.long()], torch.arange(D // 2)[:, None]].transpose(0, 1)
    else:
        cs = cos_sin[pos.long()]
    nq = (H + Hkv) * D
    x = qkv[:, :nq].float().view(T, H + Hkv, D)
    if qk_norm is not None:
        x = _qk_norm_ref(x, H, qk_norm)
    xr = _rot_ref(x, cs).to(qkv.dtype)
    qkv[:, :nq] = xr.view(T, nq)
    if slots is not None:
        v = qkv[:, nq:nq + Hkv * D].view(T, Hkv, D)
        for t in range(T):
            sl = int(slots[t])
            if sl < 0:
                continue
            blk, off = sl // KV_BLOCK, sl % KV_BLOCK
            kt, vt = xr[t, H:].float(), v[t].float()
            if k_cache.dtype == torch.float8_e4m3fn:      # the GPU writers saturate to +-448
                kt, vt = kt.clamp(-448, 448), vt.clamp(-448, 448)
            k_cache[blk, :, off, :] = kt.to(k_cache.dtype)
            v_cache[blk, :, :, off] = vt.to(v_cache.dtype)


def gather_kv(k_cache: torch.Tensor, v_cache: torch.Tensor, blocks: torch.Tensor,
              n_tokens: int) -> tuple[torch.Tensor, torch.Tensor]:
    """Token-major K and V [n_tokens, Hkv, D] of the sequence whose block list is ``blocks``
    (int64, >= ceil(n_tokens / 64) entries), copied out of the pools in the cache's dtype."""
    Hkv, D = k_cache.shape[1], k_cache.shape[3]
    kb = k_cache.index_select(0, blocks)                                  # [nb, Hkv, 64, D]
    vb = v_cache.index_select(0, blocks)                                  # [nb, Hkv, D, 64]
    return (kb.permute(0, 2, 1, 3).reshape(-1, Hkv, D)[:n_tokens],
            vb.permute(0, 3, 1, 2).reshape(-1, Hkv, D)[:n_tokens])


_DECODE_WAVES = 4            # waves (= 64-token blocks) per paged-decode workgroup (csrc/paged_attn.h PA_NW)
_DECODE_MAX_SPLITS = 32        # the in-launch split combine merges at most 32 splits per kv head


_DECODE_FEW = 4                # <= this many sequences: no minimum split size, blocks spread over every split


def decode_splits(B: int, Hkv: int, max_blocks: int, target_wg: Optional[int] = None) -> tuple[int, int]:
    """(nsplit, min blocks_per_split) of the paged decode kernel.

    A split is one workgroup of 4 waves, one 64-token block per wave.  Batched decode (B > 4):
    splits of >= 4 blocks, so a context of <= 256 tokens is one workgroup per kv head with no
    cross-workgroup combine; longer contexts use up to 32 splits merged in-launch, and past 8k
    tokens the waves loop over several blocks.  A few sequences (B <= 4): the same launch with
    no minimum, so each sequence's blocks spread over all launched splits.  The kernel sizes the
    splits from each sequence's ctx_len on the device (blocks per split = max(min,
    ceil(blocks / nsplit)))."""
    nsplit = max(1, min(-(-max_blocks // _DECODE_WAVES), _DECODE_MAX_SPLITS))
    if B <= _DECODE_FEW:
        # one block per wave, but the context spread over every launched split: 650 tokens on an
        # 8-split launch run as 6 splits x 2 blocks, 9.8 us vs 10.7 us as 3 x 4 and 20.4 us as 32
        # one-wave splits, whose single-wave combine is latency-serial (r3_decode_attn_splits_v1.txt)
        return nsplit, 1
    bps = -(-max_blocks // nsplit)
    return -(-max_blocks // bps), bps


def paged_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_table: torch.Tensor,
                 ctx_len: torch.Tensor, H: int, Hkv: int, scale: Optional[float] = None,
                 out: Optional[torch.Tensor] = None, workspace: Optional[dict] = None,
                 rope: Optional[tuple] = None, prefetch: Sequence[torch.Tensor] = (),
                 splits: Optional[tuple] = None) -> torch.Tensor:
    """Single-token attention of q [B, H*D] (rows may be views) over each sequence's cached
    context (ctx_len tokens, including the current token).

    ``rope = (pos [B] int32, cos_sin, slots [B] int64)``: q is the *unrotated* packed QKV row
    and the kernel applies RoPE to q in registers and writes the current token's rotated k and
    its v to ``slots`` itself (what :func:`rope_kv` would do; one launch per layer fewer).
    ``prefetch``: up to two tensors (the next GEMMs' weights) that extra workgroups of the same
    launch read once into the Infinity Cache while the attention occupies only a few CUs.
    Head dims 64 / 128 on the GPU."""
    B = q.shape[0]
    D = k_cache.shape[3]
    if rope is not None and not (q.is_cuda and D in (64, 128)):
        pos, cos_sin, slots = rope
        q = q.clone()
        rope_kv(q, pos, cos_sin, H, Hkv, D, slots, k_cache, v_cache)
        rope = None
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    if out is None:
        out = torch.empty((B, H * D), device=q.device, dtype=q.dtype)
    if q.is_cuda:
        mb = block_table.shape[1]
        nsplit, bps = splits if splits is not None else decode_splits(B, Hkv, mb)   # splits: benchmarks
        po = pm = None
        if nsplit > 1:
            need = B * H * nsplit
            ws = workspace if workspace is not None else {}
            po = ws.get("o")
            if po is None or po.numel() < need * D:
                po = torch.empty(need * D, device=q.device, dtype=torch.float32)
                ws["o"] = po
            pm = ws.get("ml")
            if pm is None or pm.numel() < need * 2:
                pm = torch.empty(need * 2, device=q.device, dtype=torch.float32)
                ws["ml"] = pm
        rp = (None, None, None) if rope is None else \
            (rope[0].to(torch.int32).contiguous(), rope[1], rope[2].to(torch.long).contiguous())
        pf = list(prefetch)[:2] + [None, None]
        hip_ops().paged_decode(q, k_cache, v_cache, block_table, ctx_len, out, int(H), int(Hkv), float(scale),
                               int(nsplit), int(bps), po, pm, *rp, pf[0], pf[1])
        return out
    G = H // Hkv
    for b in range(B):
        L = int(ctx_len[b])
        k, v = gather_kv(k_cache, v_cache, block_table[b, :-(-L // KV_BLOCK)].long(), L)
        k, v = k.float().permute(1, 0, 2), v.float().permute(1, 0, 2)          # [Hkv, L, D]
        qb = q[b, :H * D].float().view(Hkv, G, D)
        s = torch.einsum("hgd,htd->hgt", qb, k) * scale
        p = torch.softmax(s, -1)
        o = torch.einsum("hgt,htd->hgd", p, v)
        out[b, :H * D] = o.reshape(H * D).to(out.dtype)
    return out


PAGED_PREFILL_HEAD_DIMS = (32, 64, 128)


def paged_prefill(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, blocks: torch.Tensor,
                  start_pos: int, H: int, Hkv: int, scale: Optional[float] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Attention of T new rows of ONE sequence over its paged cache: q [T, >= H*D] (rows of the
    rotated packed QKV buffer, may be a view), ``blocks`` int64 the sequence's block list
    covering positions [0, start_pos + T).  Row i sits at position start_pos + i and attends
    cache tokens 0 .. start_pos + i; the rows' own k / v must already be in the cache
    (:func:`rope_kv` with slots).  Returns out [T, H*D].  Head dims 32 / 64 / 128 on the GPU."""
    T = q.shape[0]
    D = k_cache.shape[3]
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    if out is None:
        out = torch.empty((T, H * D), device=q.device, dtype=q.dtype)
    if q.is_cuda:
        hip_ops().paged_prefill(q, k_cache, v_cache, blocks, int(start_pos), int(H), int(Hkv), float(scale), out)
        return out
    if T == 0:
        return out
    G = H // Hkv
    S = start_pos + T
    nb = -(-S // KV_BLOCK)
    if blocks.numel() < nb:
        raise ValueError("paged_prefill: block list shorter than start_pos + T")
    k, v = gather_kv(k_cache, v_cache, blocks[:nb].long(), S)
    k, v = k.float().permute(1, 0, 2), v.float().permute(1, 0, 2)              # [Hkv, S, D]
    qb = q[:, :H * D].float().view(T, Hkv, G, D)
    s = torch.einsum("thgd,hsd->hgts", qb, k) * scale
    hidden = torch.arange(S)[None, :] > (start_pos + torch.arange(T))[:, None]       # [T, S]
    p = torch.softmax(s.masked_fill(hidden, float("-inf")), -1)
    o = torch.einsum("hgts,hsd->thgd", p, v)
    out[:, :H * D] = o.reshape(T, H * D).to(out.dtype)
    return out


PAGED_VERIFY_MAX_COLS = 64     # MFMA columns (query row, head in group) of one paged-verify workgroup


def paged_verify(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_table: torch.Tensor,
                 ctx_len: torch.Tensor, n_rows: torch.Tensor, T: int, H: int, Hkv: int,
                 scale: Optional[float] = None, out: Optional[torch.Tensor] = None,
                 workspace: Optional[dict] = None, splits: Optional[tuple] = None) -> torch.Tensor:
    """Attention of up to T new rows for each of B sequences over the paged cache in one launch
    (speculative decoding): q [B*T, >= H*D], sequence-major rows of the rotated packed QKV buffer
    (may be a view), ``block_table`` int32 [B, W], ``ctx_len`` int32 [B] the tokens in the cache
    *including* this step's rows, ``n_rows`` int32 [B] the live rows (1 .. T).  Row i of sequence b
    sits at position ctx_len[b] - n_rows[b] + i and attends cache tokens 0 .. that position; rows
    i >= n_rows[b] are padding and come out 0.  The rows' own k / v must already be in the cache
    (:func:`rope_kv` with slots).  All three per-step tensors are read on the device, so a captured
    launch replays for any step.  ``T * (H // Hkv) <= 64``.  Returns out [B*T, H*D]."""
    T = int(T)
    D = k_cache.shape[3]
    if Hkv <= 0 or H % Hkv != 0 or H // Hkv > 16:
        raise ValueError("paged_verify: at most 16 query heads per kv head")
    if T < 1 or T * (H // Hkv) > PAGED_VERIFY_MAX_COLS:
        raise ValueError(f"paged_verify: T * (H / Hkv) = {T * (H // Hkv)} exceeds {PAGED_VERIFY_MAX_COLS} columns")
    if q.dim() != 2 or q.shape[0] % T != 0 or q.shape[1] < H * D:
        raise ValueError("paged_verify: q must be [B*T, >= H*D]")
    B = q.shape[0] // T
    if block_table.dim() != 2 or block_table.shape[0] != B or ctx_len.numel() != B or n_rows.numel() != B:
        raise ValueError("paged_verify: block_table [B, W], ctx_len [B] and n_rows [B] must match q's B")
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    if out is None:
        out = torch.empty((B * T, H * D), device=q.device, dtype=q.dtype)
    elif out.dim() != 2 or out.shape[0] != B * T or out.shape[1] < H * D:
        raise ValueError("paged_verify: out must be [B*T, >= H*D]")
    if q.is_cuda:
        if D not in PAGED_PREFILL_HEAD_DIMS:
            raise ValueError("paged_verify: head dim 32, 64 or 128")
        nsplit, bps = splits if splits is not None else decode_splits(B, Hkv, block_table.shape[1])   # splits: benchmarks
        po = pm = None
        if nsplit > 1:
            need = B * T * H * nsplit
            ws = workspace if workspace is not None else {}
            po = ws.get("vo")
            if po is None or po.numel() < need * D:
                po = torch.empty(need * D, device=q.device, dtype=torch.float32)
                ws["vo"] = po
            pm = ws.get("vml")
            if pm is None or pm.numel() < need * 2:
                pm = torch.empty(need * 2, device=q.device, dtype=torch.float32)
                ws["vml"] = pm
        hip_ops().paged_verify(q, k_cache, v_cache, block_table, ctx_len, n_rows, out, T, int(H), int(Hkv),
                               float(scale), int(nsplit), int(bps), po, pm)
        return out
    G = H // Hkv
    out[:, :H * D] = 0
    for b in range(B):
        L, n = int(ctx_len[b]), min(max(int(n_rows[b]), 0), T)
        if L <= 0 or n == 0:
            continue
        k, v = gather_kv(k_cache, v_cache, block_table[b, :-(-L // KV_BLOCK)].long(), L)
        k, v = k.float().permute(1, 0, 2), v.float().permute(1, 0, 2)          # [Hkv, L, D]
        qb = q[b * T:b * T + n, :H * D].float().view(n, Hkv, G, D)
        s = torch.einsum("thgd,hsd->hgts", qb, k) * scale
        hidden = torch.arange(L)[None, :] > (L - n + torch.arange(n))[:, None]           # [n, L]
        p = torch.softmax(s.masked_fill(hidden, float("-inf")), -1)
        p = torch.nan_to_num(p)                                                # a row before position 0 sees nothing
        o = torch.einsum("hgts,hsd->thgd", p, v)
        out[b * T:b * T + n, :H * D] = o.reshape(n, H * D).to(out.dtype)
    return out


def rep_penalty_(logits: torch.Tensor, token_ids: Sequence[Sequence[int]], penalty: Sequence[float]) -> torch.Tensor:
    """logits[b, t] /= p (if > 0) or *= p for every distinct previously seen token t."""
    B = logits.shape[0]
    uniq = [sorted(set(int(t) for t in ids)) for ids in token_ids]
    maxn = max((len(u) for u in uniq), default=0)
    if maxn == 0:
        return logits
    ids = np.full((B, maxn), -1, np.int32)
    for b, u in enumerate(uniq):
        ids[b, :len(u)] = u
    if logits.is_cuda:
        hip_ops().rep_penalty_(logits, h2d(ids, logits.device), h2d(list(penalty), logits.device, torch.float32))
        return logits
    for b, u in enumerate(uniq):
        if not u:
            continue
        idx = torch.tensor(u)
        v = logits[b, idx]
        logits[b, idx] = torch.where(v > 0, v / penalty[b], v * penalty[b])
    return logits


def sample_from_candidates(vals: np.ndarray, idx: np.ndarray, lse: float, temperature: float, top_p: float,
                           rng: np.random.Generator) -> int:
    """Nucleus sampling from the top-k candidates of one row.

    ``vals`` are logits/temperature sorted descending, ``lse`` the log-sum-exp over the
    full vocabulary of the same scaled logits, so ``exp(vals - lse)`` are exact
    probabilities.  The nucleus is the smallest prefix with mass >= top_p; when the
    top-k mass is below top_p the whole candidate set is used (documented truncation)."""
    p = np.exp(vals.astype(np.float64) - lse)
    c = np.cumsum(p)
    n = int(np.searchsorted(c, top_p * c[-1] if c[-1] < top_p else top_p) + 1)
    n = max(1, min(n, len(p)))
    q = p[:n] / p[:n].sum()
    return int(idx[int(rng.choice(n, p=q))])


SAMPLE_K = 64      # candidates of the device sampler (csrc/sampler.h SAMPLE_K)


def seen_words(V: int) -> int:
    """int32 words of one row of the sampler's seen-token bitmap"""
    return -(-V // 32)


class GuideTensors(NamedTuple):
    """The guided form's tensors of :func:`sample_rows` (on the logits' device).  ``allow`` int32
    [A, ceil(V / 32)] and ``dfa`` int16 [A, 256] are the arena of grammar states of all resident
    guides (``dfa`` holds arena-global state ids, -1 = dead); ``tok_off`` int32 [V + 1] and
    ``tok_dat`` uint8 the CSR of the token bytes; ``slot`` int32 [B] the row of ``state`` a
    sequence owns (-1: an unguided row), ``g_in`` int32 [B] the state the host feeds (-1: read
    ``state[slot]``) and ``state`` int32 [S] the states kept on the device, written by the call."""
    allow: torch.Tensor
    dfa: torch.Tensor
    tok_off: torch.Tensor
    tok_dat: torch.Tensor
    slot: Any
    g_in: Any
    state: torch.Tensor


MASK_FILL_DEVICE = -1e30     # see mask_logits_


def mask_logits_(logits: torch.Tensor, allow_rows, v0: int = 0, fill: Optional[float] = None) -> torch.Tensor:
    """The host sampling path's grammar mask: ``allow_rows[b]`` is the allowed-token bitmap of row
    b's grammar state (int32 words over the whole vocabulary, bit t of word t // 32 = token t; None:
    an unguided row) and column j of ``logits`` is token ``v0 + j``.  A logit whose bit is clear is
    set to ``fill``: -inf on the CPU.  On the GPU the default is -1e30, because row_topk's online
    sum-exp must not meet -inf before a finite value; exp(-1e30 - max) is exactly 0, so the
    log-sum-exp, the finite candidates and the draw are those of the -inf form bit for bit."""
    rows = [b for b, a in enumerate(allow_rows) if a is not None]
    if not rows:
        return logits
    if fill is None:
        fill = MASK_FILL_DEVICE if logits.is_cuda else float("-inf")
    d = logits.device
    need = seen_words(v0 + logits.shape[1])       # a row shorter than the vocabulary allows nothing beyond it
    w = torch.zeros((len(rows), max(need, max(len(allow_rows[b]) for b in rows))), dtype=torch.int32)
    for k, b in enumerate(rows):
        w[k, :len(allow_rows[b])] = torch.as_tensor(np.asarray(allow_rows[b]), dtype=torch.int32)
    w = w.to(d)
    cols = torch.arange(v0, v0 + logits.shape[1], device=d)
    ok = ((w[:, cols >> 5] >> (cols & 31)) & 1).bool()
    idx = torch.as_tensor(rows, device=d)
    logits[idx] = logits[idx].masked_fill(~ok, fill)
    return logits


def sample_rows(logits: torch.Tensor, inv_t, top_p, penalty, u, greedy, seen_slot, seen: torch.Tensor, in_ids,
                out_ids: Optional[torch.Tensor] = None, candidates: bool = True, *,
                guide: Optional[GuideTensors] = None):
    """Penalise, scale, cut and draw one token per row of fp32 ``logits`` [B, V] without writing them:
    what :func:`rep_penalty_`, the 1/T multiply, ``row_topk(64)`` and :func:`sample_from_candidates`
    do in turn on the host path.

    Per row b: ``inv_t`` (1/temperature, 1 for a greedy row), ``top_p``, ``penalty``, the uniform
    ``u`` (fp64; what ``Generator.choice`` would draw), ``greedy`` (take the best candidate, ``u``
    unused) and ``seen_slot``: the row of ``seen`` (int32 [S, ceil(V / 32)], bit t = token t was
    fed before) whose tokens, with ``in_ids[b]``, are penalised; -1: no penalty.  ``in_ids[b]`` is
    then marked in that row.  ``out_ids`` (int64 [B], may be ``in_ids``) receives the tokens.

    Returns ``(v [B, 64], i [B, 64], lse [B], tok [B] int32, seen)``; ``v`` are the transformed
    logits of the candidates, descending.  ``candidates=False`` on the GPU: ``v, i, lse`` are None.
    CPU tensors run an fp32 / fp64 reference of the same operations.

    ``guide`` (:class:`GuideTensors`): the guided form.  A row with ``slot >= 0`` has the grammar
    state ``s = g_in[b]`` if that is >= 0, else ``state[slot[b]]``; the logits of the tokens whose bit
    in ``allow[s]`` is clear count as -inf before the penalty, the drawn token's bytes are walked
    through ``dfa`` from ``s`` and the result is stored in ``state[slot[b]]`` (a token without bytes
    leaves it).  A row that allows no finite logit gives ``tok = -1`` and keeps its state.  The
    result gains a sixth element, ``state``."""
    d = logits.device
    B, V = logits.shape
    as_t = lambda x, dt: torch.as_tensor(x, dtype=dt, device=d).reshape(B).contiguous()  # noqa: E731
    inv_t, penalty = as_t(inv_t, torch.float32), as_t(penalty, torch.float32)
    top_p, u = as_t(top_p, torch.float64), as_t(u, torch.float64)
    greedy, seen_slot = as_t(greedy, torch.int32), as_t(seen_slot, torch.int32)
    in_ids = as_t(in_ids, torch.long)
    if out_ids is None:
        out_ids = torch.empty(B, dtype=torch.long, device=d)
    if logits.is_cuda:
        tok = torch.empty(B, dtype=torch.int32, device=d)
        v = torch.empty((B, SAMPLE_K), dtype=torch.float32, device=d) if candidates else None
        i = torch.empty((B, SAMPLE_K), dtype=torch.int32, device=d) if candidates else None
        lse = torch.empty(B, dtype=torch.float32, device=d) if candidates else None
        if guide is not None:
            hip_ops().sample_rows(logits, inv_t, top_p, penalty, u, greedy, seen_slot, seen, in_ids, out_ids, tok,
                                  v, i, lse, guide.allow, guide.dfa, guide.tok_off, guide.tok_dat,
                                  as_t(guide.slot, torch.int32), as_t(guide.g_in, torch.int32), guide.state)
            return v, i, lse, tok, seen, guide.state
        hip_ops().sample_rows(logits, inv_t, top_p, penalty, u, greedy, seen_slot, seen, in_ids, out_ids, tok,
                              v, i, lse)
        return v, i, lse, tok, seen
    if V < SAMPLE_K:
        raise ValueError(f"sample_rows: V >= {SAMPLE_K}")
    x = logits.float().clone()
    feed = in_ids.tolist()
    shifts = torch.arange(32)
    gstate = [-1] * B        # guided rows: the grammar state the row draws in
    if guide is not None:
        gslot, gin = as_t(guide.slot, torch.int32).tolist(), as_t(guide.g_in, torch.int32).tolist()
        A, S = guide.allow.shape[0], guide.state.numel()
        for b in range(B):
            if not 0 <= gslot[b] < S:
                gslot[b] = -1
                continue
            s = gin[b] if gin[b] >= 0 else int(guide.state[gslot[b]])
            gstate[b] = s if 0 <= s < A else A
            if gstate[b] == A:
                x[b] = float("-inf")
            else:
                ok = ((guide.allow[s].long()[:, None] >> shifts) & 1).bool().reshape(-1)[:V]
                x[b, ~ok] = float("-inf")
    for b in range(B):
        slot = int(seen_slot[b])
        if slot < 0 or slot >= seen.shape[0] or float(penalty[b]) == 1.0:
            continue
        hit = ((seen[slot].long()[:, None] >> shifts) & 1).bool().reshape(-1)[:V]
        if 0 <= feed[b] < V:
            hit[feed[b]] = True
        idx = hit.nonzero().reshape(-1)
        xv = x[b, idx]
        x[b, idx] = torch.where(xv > 0, xv / penalty[b], xv * penalty[b])
    x *= inv_t[:, None]
    v, i = torch.topk(x, SAMPLE_K, dim=-1, largest=True, sorted=True)
    lse = torch.logsumexp(x, dim=-1)
    tok = torch.empty(B, dtype=torch.int32)
    vn, lsen = v.numpy(), lse.numpy()
    for b in range(B):
        j = 0
        if guide is not None and vn[b, 0] == -np.inf:      # nothing allowed (or nothing finite): no draw
            pass
        elif not int(greedy[b]):
            tp = float(top_p[b])
            c = np.cumsum(np.exp(vn[b].astype(np.float64) - np.float64(lsen[b])))
            n = int(np.searchsorted(c, tp * c[-1] if c[-1] < tp else tp) + 1)
            n = max(1, min(n, SAMPLE_K))
            j = min(n - 1, int(np.searchsorted(c[:n] / c[n - 1], float(u[b]), side="right")))
        tok[b] = -1 if guide is not None and vn[b, 0] == -np.inf else i[b, j]
        slot = int(seen_slot[b])
        if 0 <= slot < seen.shape[0] and 0 <= feed[b] < V:
            bit = 1 << (feed[b] & 31)
            seen[slot, feed[b] >> 5] |= bit - (1 << 32) if bit >> 31 else bit
    if guide is None:
        out_ids.copy_(tok.long())
        return v, i.to(torch.int32), lse, tok, seen
    off, dat = guide.tok_off.tolist(), guide.tok_dat.tolist()
    for b in range(B):
        s, t = gstate[b], int(tok[b])
        if gslot[b] < 0 or s >= A:
            continue
        ns = s
        if 0 <= t < V:
            for q in range(off[t], off[t + 1]):
                ns = int(guide.dfa[ns, dat[q]])
                if not 0 <= ns < A:
                    ns = s
                    break
        guide.state[gslot[b]] = ns
    out_ids.copy_(tok.long().clamp(min=0))
    return v, i.to(torch.int32), lse, tok, seen, guide.state


SAMPLE_VERIFY_MAX_T = 8      # rows per sequence of the sampler's verify form (csrc/sampler.h)


def _mark_seen(seen: torch.Tensor, slot: int, t: int) -> None:
    bit = 1 << (t & 31)
    seen[slot, t >> 5] |= bit - (1 << 32) if bit >> 31 else bit


def sample_verify_rows(logits: torch.Tensor, T: int, n_rows, inv_t, top_p, penalty, u, greedy, seen_slot,
                       seen: torch.Tensor, in_ids, candidates: bool = True, *,
                       guide: Optional[GuideTensors] = None):
    """The verify form of :func:`sample_rows` (speculative decoding of sampled / penalised requests):
    fp32 ``logits`` [B * T, V], row ``b * T + i`` holding the logits after input ``i`` of sequence ``b``
    -- ``in_ids[b * T]`` is its last token, the next ones its draft tokens -- and live while
    ``i < n_rows[b]``.

    ``inv_t``, ``top_p``, ``penalty``, ``greedy`` and ``seen_slot`` are per sequence [B]; ``u`` and
    ``in_ids`` per row [B * T].  Row (b, i) is penalised over the bitmap slot of b and
    ``in_ids[b * T .. b * T + i]`` (not the later inputs) and drawn as :func:`sample_rows` draws;
    a dead row gives ``tok = -1``.  The draw marks nothing.  ``n_acc[b]`` is the number of leading
    draft tokens that equal the token of the row before them (``tok[b*T + i] == in_ids[b*T + i + 1]``),
    and ``in_ids[b * T .. b * T + n_acc[b]]`` -- the tokens that really were fed -- are marked in
    the slot (a slot of -1 or beyond ``seen`` marks nothing).

    Returns ``(v [B*T, 64], i [B*T, 64], lse [B*T], tok [B*T] int32, n_acc [B] int32, seen)``; dead
    rows of ``v, i, lse`` are unspecified on the GPU (-inf, -1, 0 on the CPU).  ``candidates=False``
    on the GPU: ``v, i, lse`` are None.  CPU tensors run the reference of :func:`sample_rows` row
    by row.

    ``guide`` (:class:`GuideTensors`): the guided verify form.  ``guide.g_in`` has B * T entries:
    entry ``b * T + i`` is the grammar state (a row of ``guide.allow``) in which row (b, i) draws --
    the state after sequence b's text and its draft tokens 1 .. i, which the caller walks -- or -1
    for an unguided row.  A live row with a state is masked by the state's allow row exactly as
    :func:`mask_logits_` masks with -inf and then drawn as above; a state outside the arena allows
    nothing (``tok = -1``).  ``guide.slot`` and ``guide.state`` are ignored and left untouched (no
    state is kept between verify steps), and the result has the same six elements."""
    d = logits.device
    T = int(T)
    R, V = logits.shape
    if V < SAMPLE_K:
        raise ValueError(f"sample_verify_rows: V >= {SAMPLE_K}")
    if not 1 <= T <= SAMPLE_VERIFY_MAX_T:
        raise ValueError(f"sample_verify_rows: T in 1 .. {SAMPLE_VERIFY_MAX_T}")
    B = torch.as_tensor(n_rows).numel()
    if R != B * T:
        raise ValueError(f"sample_verify_rows: {R} rows of logits for B * T = {B} * {T}")
    as_t = lambda x, dt, n: torch.as_tensor(x, dtype=dt, device=d).reshape(n).contiguous()  # noqa: E731
    n_rows = as_t(n_rows, torch.int32, B)
    inv_t, penalty = as_t(inv_t, torch.float32, B), as_t(penalty, torch.float32, B)
    top_p, u = as_t(top_p, torch.float64, B), as_t(u, torch.float64, R)
    greedy, seen_slot = as_t(greedy, torch.int32, B), as_t(seen_slot, torch.int32, B)
    in_ids = as_t(in_ids, torch.long, R)
    if logits.is_cuda:
        tok = torch.empty(R, dtype=torch.int32, device=d)
        n_acc = torch.empty(B, dtype=torch.int32, device=d)
        v = torch.empty((R, SAMPLE_K), dtype=torch.float32, device=d) if candidates else None
        i = torch.empty((R, SAMPLE_K), dtype=torch.int32, device=d) if candidates else None
        lse = torch.empty(R, dtype=torch.float32, device=d) if candidates else None
        if guide is not None:
            g_in = as_t(guide.g_in, torch.int32, R)
            g_slot = torch.as_tensor(guide.slot, dtype=torch.int32, device=d).reshape(-1).contiguous()   # not read
            hip_ops().sample_verify_rows(logits, T, n_rows, inv_t, top_p, penalty, u, greedy, seen_slot, seen,
                                         in_ids, tok, n_acc, v, i, lse, guide.allow, guide.dfa, guide.tok_off,
                                         guide.tok_dat, g_slot, g_in, guide.state)
        else:
            hip_ops().sample_verify_rows(logits, T, n_rows, inv_t, top_p, penalty, u, greedy, seen_slot, seen,
                                         in_ids, tok, n_acc, v, i, lse)
        return v, i, lse, tok, n_acc, seen
    v = torch.full((R, SAMPLE_K), float("-inf"))
    i = torch.full((R, SAMPLE_K), -1, dtype=torch.int32)
    lse = torch.zeros(R)
    tok = torch.full((R,), -1, dtype=torch.int32)
    n_acc = torch.zeros(B, dtype=torch.int32)
    feed = in_ids.tolist()
    gin = as_t(guide.g_in, torch.int32, R).tolist() if guide is not None else [-1] * R
    one = torch.zeros(1, dtype=torch.int32)      # the row reference's state array: a scratch row per call
    for b in range(B):
        n = min(int(n_rows[b]), T)
        slot = int(seen_slot[b])
        own = 0 <= slot < seen.shape[0]
        # the row's penalty set grows by one input per row: a scratch copy of the slot, which
        # sample_rows marks with the row's input after it drew -- the real bitmap is not touched
        tmp = seen[slot:slot + 1].clone() if own else seen[:0]
        for q in range(n):
            r = b * T + q
            # a row with a state: the decode form's guided reference on that one row, fed the state
            gr = None if gin[r] < 0 else guide._replace(slot=[0], g_in=[gin[r]], state=one.clone())
            rv, ri, rl, rt, tmp = sample_rows(logits[r:r + 1], inv_t[b:b + 1], top_p[b:b + 1], penalty[b:b + 1],
                                              u[r:r + 1], greedy[b:b + 1], [0 if own else -1], tmp, in_ids[r:r + 1],
                                              guide=gr)[:5]
            v[r], i[r], lse[r], tok[r] = rv[0], ri[0], rl[0], rt[0]
        j = 0
        while j < n - 1 and int(tok[b * T + j]) == feed[b * T + j + 1]:
            j += 1
        n_acc[b] = j
        if own and n > 0:
            for t in feed[b * T:b * T + j + 1]:
                if 0 <= t < V:
                    _mark_seen(seen, slot, t)
    return v, i, lse, tok, n_acc, seen
