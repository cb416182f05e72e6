"""Sparse mixture-of-experts MLP (Qwen3-MoE): routing, grouped expert GEMMs, weighted combine.

GPU tensors run the HIP kernels of csrc/moe.hip -- router logits and top-k, a stable counting sort
of the (token, choice) pairs by expert, the two grouped GEMMs with the SwiGLU epilogue and the
combine -- with no host read and launches sized from (T, E, k, H, I) alone, so the whole MLP can be
captured into a decode graph.  CPU tensors run the fp32 PyTorch reference with the same semantics.

Layouts: ``gate_w`` [E, H]; ``gu_w`` [E, 2I, H], every expert's gate and up projections interleaved
by :func:`lumen_amd.ops.glu_interleave` (8 gate | 8 up rows per 16); ``down_w`` [E, H, I].

Expert weight formats, told by the dtype of ``gu_w`` / ``down_w`` (the convention of ``ops.linear``'s
``w_scale``): the activation dtype (bf16 on the GPU); ``float8_e4m3fn`` codes with fp32 scales per output
row, ``gu_s`` [E, 2I] and ``down_s`` [E, H] (csrc/moe_wq.hip; H and I multiples of 64); ``uint8`` 4-bit
codes [E, N, K / 2] with fp16 (scale, wmin) per group, ``gu_s`` [E, 2I, H / G, 2] and ``down_s``
[E, H, I / G, 2], G = ``ops.w4_group(K)``.  The router always reads ``gate_w`` in the activation dtype.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from .._native import hip_ops
from . import dequantize_w4, w4_group

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


def _weight_format(w: torch.Tensor) -> str:
    return "fp8" if w.dtype == torch.float8_e4m3fn else "w4" if w.dtype == torch.uint8 else "float"


def _check_qweight(name: str, fmt: str, w: torch.Tensor, s: Optional[torch.Tensor], E: int, N: int, K: int,
                   x: torch.Tensor) -> None:
    """Codes ``w`` and scales / group parameters ``s`` of E matrices [N, K] in format ``fmt``."""
    if fmt == "float":
        if s is not None:
            raise ValueError(f"moe: {name} is not quantised but scales were given")
        if tuple(w.shape) != (E, N, K) or w.dtype != x.dtype:
            raise ValueError(f"moe: {name} must be [{E}, {N}, {K}] of x's dtype, got {tuple(w.shape)} {w.dtype}")
    else:
        if s is None:
            raise ValueError(f"moe: {name} holds {fmt} codes and needs its scales")
        if fmt == "fp8":
            if K % 64:
                raise ValueError(f"moe: fp8 experts need H % 64 == 0 and I % 64 == 0, got K = {K} for {name}")
            wshape, sshape, sdtype = (E, N, K), (E, N), torch.float32
        else:
            if K % 32:
                raise ValueError(f"moe: 4-bit experts need K % 32 == 0, got K = {K} for {name}")
            wshape, sshape, sdtype = (E, N, K // 2), (E, N, K // w4_group(K), 2), torch.float16
        if tuple(w.shape) != wshape:
            raise ValueError(f"moe: {name} must be {fmt} codes {wshape}, got {tuple(w.shape)}")
        if tuple(s.shape) != sshape or s.dtype != sdtype or s.device != x.device or not s.is_contiguous():
            raise ValueError(f"moe: the scales of {name} must be contiguous {sdtype} {sshape} on x's device, got "
                             f"{tuple(s.shape)} {s.dtype}")
    if not w.is_contiguous() or w.device != x.device:
        raise ValueError(f"moe: {name} must be contiguous and on x's device")


def _check_weights(x: torch.Tensor, gu_w: torch.Tensor, down_w: torch.Tensor, gu_s: Optional[torch.Tensor] = None,
                   down_s: Optional[torch.Tensor] = None) -> str:
    """Shapes, formats and scales of the expert weights; returns the format ("float", "fp8", "w4")."""
    if x.dim() != 2 or gu_w.dim() != 3 or down_w.dim() != 3:
        raise ValueError("moe: x [T, H], gu_w [E, 2I, H], down_w [E, H, I]")
    H = x.shape[1]
    E, I = gu_w.shape[0], gu_w.shape[1] // 2
    fmt = _weight_format(gu_w)
    if _weight_format(down_w) != fmt:
        raise ValueError(f"moe: gu_w ({gu_w.dtype}) and down_w ({down_w.dtype}) must have one weight format")
    if H % 32 or I % 32 or I <= 0:
        raise ValueError(f"moe: H % 32 == 0 and I % 32 == 0, got H = {H}, I = {I}")
    if not 1 <= E <= MAX_EXPERTS:
        raise ValueError(f"moe: 1 <= E <= {MAX_EXPERTS}, got E = {E}")
    if gu_w.shape[1] != 2 * I or down_w.shape[0] != E:
        raise ValueError(f"moe: gu_w [E, 2I, H] and down_w [E, H, I] must agree with x [T, H]: got "
                         f"{tuple(gu_w.shape)}, {tuple(down_w.shape)}, H = {H}")
    _check_qweight("gu_w", fmt, gu_w, gu_s, E, 2 * I, H, x)
    _check_qweight("down_w", fmt, down_w, down_s, E, H, I, x)
    return fmt


def _check_experts(x: torch.Tensor, ids: torch.Tensor, w: torch.Tensor, gu_w: torch.Tensor, down_w: torch.Tensor,
                   residual: Optional[torch.Tensor], out: Optional[torch.Tensor], gu_s: Optional[torch.Tensor] = None,
                   down_s: Optional[torch.Tensor] = None) -> str:
    fmt = _check_weights(x, gu_w, down_w, gu_s, down_s)
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
    return fmt


def _dequant_expert(fmt: str, w: torch.Tensor, s: Optional[torch.Tensor], e: int) -> torch.Tensor:
    """Expert ``e``'s matrix in fp32: the definition of what the quantised formats mean."""
    if fmt == "fp8":
        return w[e].float() * s[e].float()[:, None]
    if fmt == "w4":
        return dequantize_w4(w[e], s[e])
    return w[e].float()


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
                residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, *,
                gu_s: Optional[torch.Tensor] = None, down_s: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[t] = residual[t] + sum_j w[t, j] * down_e(silu(gate_e x_t) * up_e x_t) with e = ids[t, j],
    summed in fp32 in j order and rounded once.  ``ids`` int32 [T, k] come from the caller (usually
    :func:`moe_route`); a pair whose id lies outside [0, E) contributes nothing.  ``residual`` may be
    ``out``.  H and I must be multiples of 32 (fp8 experts: of 64).  ``gu_s`` / ``down_s`` are the scales
    or group parameters of quantised experts (module docstring); the CPU path dequantises every used
    expert in fp32 and runs the same reference.  The GPU path allocates its workspace per call: g bf16
    [T k, I] and y fp32 [T k, H], linear in T (159 MB at T = 2048 of the Qwen3-30B-A3B layer), and groups
    the T k <= 2^20 pairs in one workgroup: chunk a long prefill."""
    fmt = _check_experts(x, ids, w, gu_w, down_w, residual, out, gu_s, down_s)
    T, H = x.shape
    E, I = gu_w.shape[0], gu_w.shape[1] // 2
    if out is None:
        out = torch.empty((T, H), device=x.device, dtype=x.dtype)
    if x.is_cuda:
        if x.stride(-1) != 1 or x.stride(0) % 8 != 0:
            x = x.contiguous()
        if fmt == "float":
            hip_ops().moe_experts(x, ids.contiguous(), w.contiguous(), gu_w, down_w, residual, out)
        else:
            hip_ops().moe_experts_q(x, ids.contiguous(), w.contiguous(), gu_w, gu_s, down_w, down_s, residual, out)
        return out
    xf = x.float()
    k = ids.shape[1]
    y = torch.zeros((T, k, H), dtype=torch.float32)
    idl = ids.long()
    for e in range(E):
        t_idx, j_idx = torch.nonzero(idl == e, as_tuple=True)
        if t_idx.numel() == 0:
            continue
        gu = (xf[t_idx] @ _dequant_expert(fmt, gu_w, gu_s, e).t()).view(-1, 2 * I // 16, 2, 8)
        g = (F.silu(gu[:, :, 0]) * gu[:, :, 1]).reshape(-1, I)
        y[t_idx, j_idx] = g @ _dequant_expert(fmt, down_w, down_s, e).t()
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
            out: Optional[torch.Tensor] = None, *, gu_s: Optional[torch.Tensor] = None,
            down_s: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The sparse MLP of one layer: :func:`moe_route` then :func:`moe_experts` (``gu_s`` / ``down_s``:
    the scales of quantised experts; the router stays in the activation dtype)."""
    if gate_w.dim() == 2 and gu_w.dim() == 3 and gate_w.shape[0] != gu_w.shape[0]:
        raise ValueError(f"moe: gate_w has {gate_w.shape[0]} experts, gu_w {gu_w.shape[0]}")
    _check_route(x, gate_w, int(k))
    _check_weights(x, gu_w, down_w, gu_s, down_s)            # every check before the first launch
    for name, t in (("residual", residual), ("out", out)):
        if t is not None and (tuple(t.shape) != tuple(x.shape) or t.dtype != x.dtype or t.device != x.device):
            raise ValueError(f"moe: {name} must be [T, H] of x's dtype on x's device")
    ids, w = moe_route(x, gate_w, k, norm_topk)
    return moe_experts(x, ids, w, gu_w, down_w, residual=residual, out=out, gu_s=gu_s, down_s=down_s)


def moe_grouped_linear(x: torch.Tensor, ids: torch.Tensor, W: torch.Tensor,
                       w_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One grouped GEMM with nothing around it: x [T, K], ids int32 [T, k], W [E, N, K] in any expert
    format (``w_scale``: its scales [E, N] or group parameters [E, N, K / G, 2]) -> fp32 [T, k, N] with
    out[t, j] = x[t] . W[ids[t, j]]^T.  Pairs whose id lies outside [0, E) come back zero.  On the GPU:
    the grouping plus the down-projection kernel with the gather through the sorted order as its row
    map, gathered back pair by pair.  N must be a multiple of 16 there."""
    if x.dim() != 2 or ids.dim() != 2 or W.dim() != 3 or ids.shape[0] != x.shape[0]:
        raise ValueError("moe: x [T, K], ids [T, k], W [E, N, K]")
    if ids.dtype != torch.int32 or ids.device != x.device:
        raise ValueError("moe: ids int32 on x's device")
    T, K = x.shape
    E, N, k = W.shape[0], W.shape[1], ids.shape[1]
    if not 1 <= E <= MAX_EXPERTS or k < 1 or T * k > MAX_PAIRS:
        raise ValueError(f"moe: 1 <= E <= {MAX_EXPERTS}, 1 <= k and T * k <= {MAX_PAIRS}")
    if K % 32:
        raise ValueError(f"moe: K % 32 == 0, got K = {K}")
    fmt = _weight_format(W)
    _check_qweight("W", fmt, W, w_scale, E, N, K, x)
    if x.is_cuda:
        if x.dtype != torch.bfloat16:
            raise ValueError("moe: the HIP kernels take bf16 tensors")
        if N % 16:
            raise ValueError(f"moe: N % 16 == 0 on the GPU, got N = {N}")
        if x.stride(-1) != 1 or x.stride(0) % 8 != 0:
            x = x.contiguous()
        y, pos = hip_ops().moe_grouped_linear(x, ids.contiguous(), W, w_scale)
        if T == 0:
            return y.view(0, k, N)
        rows = y.index_select(0, pos.clamp_min(0).long())
        return torch.where((pos >= 0)[:, None], rows, torch.zeros((), device=x.device)).view(T, k, N)
    out = torch.zeros((T, k, N), dtype=torch.float32)
    xf, idl = x.float(), ids.long()
    for e in range(E):
        t_idx, j_idx = torch.nonzero(idl == e, as_tuple=True)
        if t_idx.numel():
            out[t_idx, j_idx] = xf[t_idx] @ _dequant_expert(fmt, W, w_scale, e).t()
    return out
