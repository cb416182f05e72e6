"""Sparse mixture-of-experts MLP (Qwen3-MoE): routing, grouped expert GEMMs, weighted combine.

GPU tensors run the HIP kernels of csrc/moe.hip -- router logits and top-k, a stable counting sort
of the (token, choice) pairs by expert, the two grouped GEMMs with the SwiGLU epilogue and the
combine -- with no host read and launches sized from (T, E, k, H, I) alone, so the whole MLP can be
captured into a decode graph.  CPU tensors run the fp32 PyTorch reference with the same semantics.

Layouts: ``gate_w`` [E, H]; ``gu_w`` [E, 2I, H], every expert's gate and up projections interleaved
by :func:`lumen_amd.ops.glu_interleave` (8 gate | 8 up rows per 16); ``down_w`` [E, H, I].
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from .._native import hip_ops

MAX_EXPERTS = 256
MAX_TOPK = 8
MAX_PAIRS = 1 << 20      # T * k of one call (csrc/moe.h)


def _check_route(x: torch.Tensor, gate_w: torch.Tensor, k: int) -> None:
    if x.dim() != 2 or gate_w.dim() != 2 or gate_w.shape[1] != x.shape[1]:
        raise ValueError(f"moe: x [T, H] and gate_w [E, H], got {tuple(x.shape)} and {tuple(gate_w.shape)}")
    E, H = gate_w.shape
    if not 1 <= E <= MAX_EXPERTS:
        raise ValueError(f"moe: 1 <= E <= {MAX_EXPERTS}, got E = {E}")
    if not 1 <= k <= min(E, MAX_TOPK):
        raise ValueError(f"moe: 1 <= k <= min(E, {MAX_TOPK}), got k = {k} with E = {E}")
    if H % 32:
        raise ValueError(f"moe: H % 32 == 0, got H = {H}")
    if x.shape[0] * k > MAX_PAIRS:
        raise ValueError(f"moe: T * k <= {MAX_PAIRS} (chunk a longer prefill), got {x.shape[0] * k}")
    if gate_w.dtype != x.dtype or gate_w.device != x.device:
        raise ValueError("moe: gate_w must have x's dtype and device")
    if x.is_cuda and x.dtype != torch.bfloat16:
        raise ValueError("moe: the HIP kernels take bf16 tensors")


def _check_weights(x: torch.Tensor, gu_w: torch.Tensor, down_w: torch.Tensor) -> None:
    if x.dim() != 2 or gu_w.dim() != 3 or down_w.dim() != 3:
        raise ValueError("moe: x [T, H], gu_w [E, 2I, H], down_w [E, H, I]")
    H = x.shape[1]
    E, I = gu_w.shape[0], down_w.shape[2]
    if H % 32 or I % 32:
        raise ValueError(f"moe: H % 32 == 0 and I % 32 == 0, got H = {H}, I = {I}")
    if not 1 <= E <= MAX_EXPERTS:
        raise ValueError(f"moe: 1 <= E <= {MAX_EXPERTS}, got E = {E}")
    if tuple(gu_w.shape) != (E, 2 * I, H) or tuple(down_w.shape) != (E, H, I):
        raise ValueError(f"moe: gu_w [E, 2I, H] and down_w [E, H, I] must agree with x [T, H]: got "
                         f"{tuple(gu_w.shape)}, {tuple(down_w.shape)}, H = {H}")
    for name, t in (("gu_w", gu_w), ("down_w", down_w)):
        if t.dtype != x.dtype or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"moe: {name} must be contiguous, of x's dtype and on x's device")


def _check_experts(x: torch.Tensor, ids: torch.Tensor, w: torch.Tensor, gu_w: torch.Tensor, down_w: torch.Tensor,
                   residual: Optional[torch.Tensor], out: Optional[torch.Tensor]) -> None:
    _check_weights(x, gu_w, down_w)
    T, H = x.shape
    E = gu_w.shape[0]
    if ids.dim() != 2 or ids.shape[0] != T or tuple(w.shape) != tuple(ids.shape):
        raise ValueError(f"moe: ids and w [T, k], got {tuple(ids.shape)} and {tuple(w.shape)} for T = {T}")
    if not 1 <= ids.shape[1] <= min(E, MAX_TOPK):
        raise ValueError(f"moe: 1 <= k <= min(E, {MAX_TOPK}), got k = {ids.shape[1]} with E = {E}")
    if ids.dtype != torch.int32 or w.dtype != torch.float32:
        raise ValueError("moe: ids int32 and w float32")
    for name, t in (("residual", residual), ("out", out)):
        if t is not None and (tuple(t.shape) != (T, H) or t.dtype != x.dtype):
            raise ValueError(f"moe: {name} must be [T, H] of x's dtype")
    for name, t in (("ids", ids), ("w", w), ("residual", residual), ("out", out)):
        if t is not None and t.device != x.device:
            raise ValueError(f"moe: {name} is on {t.device}, x on {x.device}")
    if x.is_cuda and x.dtype != torch.bfloat16:
        raise ValueError("moe: the HIP kernels take bf16 tensors")


def route_weights(logits: torch.Tensor, ids: torch.Tensor, norm_topk: bool = True) -> torch.Tensor:
    """fp32 routing weights of the chosen experts ``ids`` [T, k] given the router logits [T, E]:
    the softmax over the k chosen logits (``norm_topk``) or exp(l_j - logsumexp(l over all E))."""
    lf = logits.float()
    sel = lf.gather(1, ids.long())
    if norm_topk:
        return torch.softmax(sel, dim=1)
    return torch.exp(sel - torch.logsumexp(lf, dim=1, keepdim=True))


def moe_route(x: torch.Tensor, gate_w: torch.Tensor, k: int, norm_topk: bool = True) -> tuple[torch.Tensor, torch.Tensor]:
    """Router of a sparse MLP: x [T, H] rows (already normalised), gate_w [E, H] -> (ids int32 [T, k],
    w fp32 [T, k]).  fp32 logits, the top k over E in descending order with ties going to the lower
    expert id, weights as in :func:`route_weights`.  E <= 256, 1 <= k <= min(E, 8)."""
    k = int(k)
    _check_route(x, gate_w, k)
    if x.is_cuda:
        if x.stride(-1) != 1 or x.stride(0) % 8 != 0:
            x = x.contiguous()
        ids, w = hip_ops().moe_route(x, gate_w.contiguous(), k, bool(norm_topk))
        return ids, w
    logits = x.float() @ gate_w.float().t()
    ids = torch.sort(logits, dim=1, descending=True, stable=True).indices[:, :k]
    return ids.to(torch.int32), route_weights(logits, ids, norm_topk)


def moe_experts(x: torch.Tensor, ids: torch.Tensor, w: torch.Tensor, gu_w: torch.Tensor, down_w: torch.Tensor,
                residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[t] = residual[t] + sum_j w[t, j] * down_e(silu(gate_e x_t) * up_e x_t) with e = ids[t, j],
    summed in fp32 in j order and rounded once.  ``ids`` int32 [T, k] come from the caller (usually
    :func:`moe_route`); a pair whose id lies outside [0, E) contributes nothing.  ``residual`` may be
    ``out``.  H and I must be multiples of 32.  The GPU path allocates its workspace per call: g bf16
    [T k, I] and y fp32 [T k, H], linear in T (159 MB at T = 2048 of the Qwen3-30B-A3B layer), and groups
    the T k <= 2^20 pairs in one workgroup: chunk a long prefill."""
    _check_experts(x, ids, w, gu_w, down_w, residual, out)
    T, H = x.shape
    E, I = gu_w.shape[0], down_w.shape[2]
    if out is None:
        out = torch.empty((T, H), device=x.device, dtype=x.dtype)
    if x.is_cuda:
        if x.stride(-1) != 1 or x.stride(0) % 8 != 0:
            x = x.contiguous()
        hip_ops().moe_experts(x, ids.contiguous(), w.contiguous(), gu_w, down_w, residual, out)
        return out
    xf = x.float()
    k = ids.shape[1]
    y = torch.zeros((T, k, H), dtype=torch.float32)
    idl = ids.long()
    for e in range(E):
        t_idx, j_idx = torch.nonzero(idl == e, as_tuple=True)
        if t_idx.numel() == 0:
            continue
        gu = (xf[t_idx] @ gu_w[e].float().t()).view(-1, 2 * I // 16, 2, 8)
        g = (F.silu(gu[:, :, 0]) * gu[:, :, 1]).reshape(-1, I)
        y[t_idx, j_idx] = g @ down_w[e].float().t()
    acc = torch.zeros((T, H), dtype=torch.float32)
    valid = (idl >= 0) & (idl < E)
    for j in range(k):
        acc = acc + torch.where(valid[:, j:j + 1], w[:, j:j + 1].float() * y[:, j], torch.zeros(()))
    if residual is not None:
        acc = acc + residual.float()
    out.copy_(acc.to(out.dtype))
    return out


def moe_mlp(x: torch.Tensor, gate_w: torch.Tensor, gu_w: torch.Tensor, down_w: torch.Tensor, k: int,
            norm_topk: bool = True, residual: Optional[torch.Tensor] = None,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The sparse MLP of one layer: :func:`moe_route` then :func:`moe_experts`."""
    if gate_w.dim() == 2 and gu_w.dim() == 3 and gate_w.shape[0] != gu_w.shape[0]:
        raise ValueError(f"moe: gate_w has {gate_w.shape[0]} experts, gu_w {gu_w.shape[0]}")
    _check_route(x, gate_w, int(k))
    _check_weights(x, gu_w, down_w)            # every check before the first launch
    for name, t in (("residual", residual), ("out", out)):
        if t is not None and (tuple(t.shape) != tuple(x.shape) or t.dtype != x.dtype or t.device != x.device):
            raise ValueError(f"moe: {name} must be [T, H] of x's dtype on x's device")
    ids, w = moe_route(x, gate_w, k, norm_topk)
    return moe_experts(x, ids, w, gu_w, down_w, residual=residual, out=out)
