"""Per-head q / k RMSNorm (Qwen3) inside the RoPE + KV-write kernels (csrc/llm.hip, per-element and
tile form) vs the fp32 CPU reference of ops/llm.py.

Inputs are drawn as in test_llm_ops_gpu.py (randn QKV rows in bf16, random positions below 4000,
shuffled slots with one -1); q_gamma and k_gamma are drawn independently, uniform in [0.5, 1.5] per
element, so a q / k swap, a gamma indexed by the pair index alone and an ignored gamma all show.

Bounds (test_llm_ops_gpu.py's): rotated q and a bf16 K cache within 0.05 absolute of the reference.
The reference rounds to bf16 once, after the rotation; the kernels compute the same fp32 expression
with another summation order for the sum of squares, so a result differs from the reference by at
most one bf16 step where the fp32 values straddle a rounding boundary.  Every case asserts that
the reference stays below 8 in magnitude, where one bf16 step is 2^-5 = 0.031 < 0.05."""
import pytest
import torch

from lumen_amd._native import hip_ops
from lumen_amd.ops import llm

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-6


def _gammas(D, g):
    return torch.rand(D, generator=g) + 0.5, torch.rand(D, generator=g) + 0.5


def _dev_norm(qg, kg):
    return qg.to(DEV), kg.to(DEV), EPS


def _cache(NB, Hkv, D, g, fp8):
    k = torch.randn(NB, Hkv, 64, D, generator=g).bfloat16()
    v = torch.randn(NB, Hkv, D, 64, generator=g).bfloat16()
    return (k.to(torch.float8_e4m3fn), v.to(torch.float8_e4m3fn)) if fp8 else (k, v)


def _check_rope_kv(T, H, Hkv, D, fp8, pos, slots, NB, seed):
    g = torch.Generator().manual_seed(seed)
    x32 = torch.randn(T, (H + 2 * Hkv) * D, generator=g)
    qkv = x32.bfloat16()
    cs = llm.rope_cos_sin(4096, D, 1e6)
    qg, kg = _gammas(D, g)
    kc, vc = _cache(NB, Hkv, D, g, fp8)
    nq = (H + Hkv) * D
    q_ref, kc_ref, vc_ref = qkv.clone(), kc.clone(), vc.clone()
    llm.rope_kv(q_ref, pos, cs, H, Hkv, D, slots, kc_ref, vc_ref, qk_norm=(qg, kg, EPS))
    # the bounds' premises: the reference on the bf16-rounded inputs stays within 0.05 of its own
    # fp32 result, and below 8 in magnitude (one bf16 step < 0.05)
    q_32 = x32.clone()
    llm.rope_kv(q_32, pos, cs, H, Hkv, D, qk_norm=(qg, kg, EPS))
    assert (q_ref[:, :nq].float() - q_32[:, :nq]).abs().max().item() < 0.05
    assert q_ref[:, :nq].float().abs().max().item() < 8.0
    assert torch.equal(q_ref[:, nq:], qkv[:, nq:])
    # gammas matter: the reference moves by far more than the bound when they are ignored
    q_one = qkv.clone()
    llm.rope_kv(q_one, pos, cs, H, Hkv, D, qk_norm=(torch.ones(D), torch.ones(D), EPS))
    assert (q_one.float() - q_ref.float()).abs().max().item() > 0.5

    q_g, kc_g, vc_g = qkv.clone().to(DEV), kc.clone().to(DEV), vc.clone().to(DEV)
    llm.rope_kv(q_g, pos.to(DEV), cs.to(DEV), H, Hkv, D, slots.to(DEV), kc_g, vc_g, qk_norm=_dev_norm(qg, kg))
    dq = (q_g.cpu().float() - q_ref.float()).abs()
    dk = (kc_g.cpu().float() - kc_ref.float()).abs()
    print(f"rope_kv+norm T={T} H={H} Hkv={Hkv} D={D} fp8={fp8}: max dq {dq.max().item():.4f} "
          f"max dk {dk.max().item():.4f} differing k {(dk > 0).float().mean().item():.4f}")
    assert dq.max().item() < 0.05
    assert torch.equal(q_g.cpu()[:, nq:], qkv[:, nq:])              # v columns of the rows untouched
    if fp8:     # one e4m3 step where the rotated bf16 value itself differs by a step
        assert (dk <= 0.13 * kc_ref.float().abs() + 1e-3).all() and (dk > 0).float().mean().item() < 0.02
        assert torch.equal(vc_g.cpu().view(torch.uint8), vc_ref.view(torch.uint8))
    else:
        assert dk.max().item() < 0.05
        assert torch.equal(vc_g.cpu(), vc_ref)
    # the written rows are the normalised ones (not the cache's initial contents)
    live = slots[slots >= 0]
    written = kc_g.cpu().float()[live // 64, :, live % 64]
    assert (written - kc.float()[live // 64, :, live % 64]).abs().max().item() > 0.5


# T < 64: the per-element kernel.  (4, 2, 64): 192 pairs in one 256-thread block, the last two
# 32-lane segments past the bound; (5, 1, 128): 384 pairs, two blocks, the second half full;
# (4, 2, 32): 16-lane segments; T = 33: more rows than a wave has segments
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("T,H,Hkv,D", [(3, 4, 2, 64), (3, 5, 1, 128), (3, 4, 2, 32), (33, 4, 2, 64)])
def test_rope_kv_norm_per_element(T, H, Hkv, D, fp8):
    g = torch.Generator().manual_seed(T + H + D)
    pos = torch.randint(0, 4000, (T,), generator=g, dtype=torch.int32)
    slots = torch.randperm(2 * 64, generator=g)[:T].long()
    slots[1] = -1
    _check_rope_kv(T, H, Hkv, D, fp8, pos, slots, 2, seed=100 + T + H + D)


# T = 70: one full 64-row tile plus a ragged tile of 6 rows, the slots running through the blocks
# from an unaligned start
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("H,Hkv,D", [(4, 2, 64), (3, 1, 128)])
def test_rope_kv_norm_tiles(H, Hkv, D, fp8):
    T, start = 70, 37
    pos = torch.arange(start, start + T, dtype=torch.int32)
    table = torch.tensor([2, 0, 1])
    p = torch.arange(start, start + T)
    slots = (table[p // 64] * 64 + p % 64).long()
    _check_rope_kv(T, H, Hkv, D, fp8, pos, slots, 3, seed=200 + H + D)


def test_no_norm_calls_are_unchanged():
    """qk_norm=None is the call without the argument, bit for bit, for the per-element and the tile
    kernel, and for the raw op called with its previous argument list."""
    H, Hkv, D = 4, 2, 64
    g = torch.Generator().manual_seed(5)
    cs = llm.rope_cos_sin(4096, D, 1e6).to(DEV)
    for T in (5, 70):                                              # per-element and tile kernels
        qkv = torch.randn(T, (H + 2 * Hkv) * D, generator=g).bfloat16()
        pos = torch.randint(0, 4000, (T,), generator=g, dtype=torch.int32).to(DEV)
        slots = torch.randperm(2 * 64, generator=g)[:T].long()
        slots[2] = -1
        kc, vc = _cache(2, Hkv, D, g, False)
        outs = []
        for mode in ("omitted", "none", "raw"):
            q, k, v = qkv.to(DEV), kc.to(DEV), vc.to(DEV)
            if mode == "omitted":
                llm.rope_kv(q, pos, cs, H, Hkv, D, slots.to(DEV), k, v)
            elif mode == "none":
                llm.rope_kv(q, pos, cs, H, Hkv, D, slots.to(DEV), k, v, qk_norm=None)
            else:
                hip_ops().rope_kv(q, pos, cs, slots.to(DEV), k, v, H, Hkv, D)
            outs.append((q, k, v))
        for o in outs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))


def test_norm_argument_errors():
    H, Hkv, D = 4, 2, 64
    g = torch.Generator().manual_seed(6)
    qg, kg = _gammas(D, g)
    qkv = torch.randn(1, (H + 2 * Hkv) * D, generator=g).bfloat16().to(DEV)
    cs = llm.rope_cos_sin(64, D, 1e6).to(DEV)
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="qk norm"):             # gammas of another length
        llm.rope_kv(qkv.clone(), pos, cs, H, Hkv, D, qk_norm=(qg[:32].to(DEV), kg[:32].to(DEV), EPS))
    with pytest.raises(RuntimeError, match="qk norm"):             # half-precision gammas
        llm.rope_kv(qkv.clone(), pos, cs, H, Hkv, D, qk_norm=(qg.to(DEV).bfloat16(), kg.to(DEV).bfloat16(), EPS))
    with pytest.raises(RuntimeError, match="qk norm"):             # one gamma without the other
        hip_ops().rope_kv(qkv.clone(), pos, cs, None, qkv, qkv, H, Hkv, D, qg.to(DEV), None, EPS)
