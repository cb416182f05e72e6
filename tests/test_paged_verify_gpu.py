"""Paged-verify attention kernel (csrc/llm.hip: up to T new query rows for each of B sequences over
the paged KV pools, one launch) vs its fp32 CPU reference and vs the paged-decode kernel."""
import pytest
import torch

from lumen_amd.ops import llm

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
# first-row positions of the mixed batch: the start; rows straddling a block edge; a block start;
# several context splits; more than 32 blocks (the waves loop where the launch has few splits)
FIRST_POS = (1, 62, 64, 650, 2100)


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-6)).item()


def _case(H, Hkv, D, T, dtype, seed, first_pos=FIRST_POS):
    """CPU tensors of one launch: a sequence per first-row position with n_rows 1, T, T - 1, ...
    plus one padded sequence (ctx 1, n_rows 1, block 0); shuffled block lists; every pool slot that
    is not a live token NaN (bf16 0x7FC0 / e4m3fn 0x7F); packed QKV rows as a strided view."""
    g = torch.Generator().manual_seed(seed)
    cyc = [1, T] + [max(1, T - 1 - i) for i in range(len(first_pos))]
    n_rows = [min(T, cyc[i]) for i in range(len(first_pos))] + [1]
    ctx = [p + n for p, n in zip(first_pos, n_rows)] + [1]
    B = len(ctx)
    nbs = [-(-c // 64) for c in ctx[:-1]]
    W = max(nbs) + 1
    NB = sum(nbs) + 4                                       # block 0 (the padded sequence's) + spares, all NaN
    perm = (torch.randperm(NB - 1, generator=g) + 1).int()
    raw, nan = (torch.uint8, 0x7F) if dtype == FP8 else (torch.int16, 0x7FC0)
    kc = torch.full((NB, Hkv, 64, D), nan, dtype=raw)
    vc = torch.full((NB, Hkv, D, 64), nan, dtype=raw)
    bt = torch.zeros((B, W), dtype=torch.int32)
    used = 0
    for b, (c, nb) in enumerate(zip(ctx[:-1], nbs)):
        blocks = perm[used:used + nb]
        used += nb
        bt[b, :nb] = blocks
        bt[b, nb:] = NB + 5                                 # beyond the live blocks: never read
        for pool, transposed in ((kc, False), (vc, True)):
            vals = torch.randn(c, Hkv, D, generator=g).to(dtype).view(raw)
            full = torch.full((nb * 64, Hkv, D), nan, dtype=raw)
            full[:c] = vals
            full = full.view(nb, 64, Hkv, D)
            pool[blocks.long()] = full.permute(0, 2, 3, 1) if transposed else full.permute(0, 2, 1, 3)
    kc[0, :, 0, :] = torch.randn(Hkv, D, generator=g).to(dtype).view(raw)       # the padded sequence's one token
    vc[0, :, :, 0] = torch.randn(Hkv, D, generator=g).to(dtype).view(raw)
    qbuf = torch.randn(B * T, (H + 2 * Hkv) * D + 8, generator=g).bfloat16()
    return (qbuf, kc.view(dtype), vc.view(dtype), bt, torch.tensor(ctx, dtype=torch.int32),
            torch.tensor(n_rows, dtype=torch.int32))


def _rows(qbuf):
    """the packed QKV rows as a view whose row stride is not its width"""
    q = qbuf[:, :qbuf.shape[1] - 8]
    assert q.stride(0) == q.shape[1] + 8 and q.data_ptr() == qbuf.data_ptr()
    return q


def _gpu(case):
    return tuple(t.to(DEV) for t in case)


SHAPES = [(14, 2, 64), (32, 8, 128), (4, 4, 64), (16, 1, 64)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, FP8], ids=["bf16", "fp8"])
@pytest.mark.parametrize("T", [1, 2, 4, 8])
@pytest.mark.parametrize("H,Hkv,D", SHAPES)
def test_paged_verify_vs_cpu_reference(H, Hkv, D, T, dtype):
    case = _case(H, Hkv, D, T, dtype, seed=H * D + T)
    qbuf, kc, vc, bt, ctx, n_rows = case
    if T * (H // Hkv) > 64:
        gq, gk, gv, gbt, gctx, gn = _gpu(case)
        with pytest.raises(ValueError, match="columns"):
            llm.paged_verify(_rows(gq), gk, gv, gbt, gctx, gn, T, H, Hkv)
        return
    assert not torch.isfinite(kc.float()).all() and not torch.isfinite(vc.float()).all()   # the NaN slots are there
    ref = llm.paged_verify(_rows(qbuf), kc, vc, bt.clamp(max=kc.shape[0] - 1), ctx, n_rows, T, H, Hkv)
    R = qbuf.shape[0]
    assert ref.shape == (R, H * D) and torch.isfinite(ref.float()).all(), "the reference must not see the NaN slots"
    guard = torch.full((R + 2, H * D), 777.0, dtype=torch.bfloat16, device=DEV)
    out = guard[1:R + 1]
    gq, gk, gv, gbt, gctx, gn = _gpu(case)
    got = llm.paged_verify(_rows(gq), gk, gv, gbt, gctx, gn, T, H, Hkv, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.isfinite(got.float()).all()
    assert (guard[0] == 777.0).all() and (guard[R + 1] == 777.0).all(), "guard rows overwritten"
    for b in range(len(ctx)):
        pad = got[b * T + int(n_rows[b]):(b + 1) * T]
        assert (pad == 0).all(), "padding rows come out zero"
    err = _rel(got, ref)
    print(f"paged_verify H={H} Hkv={Hkv} D={D} T={T} {dtype}: rel err {err:.3e}")
    assert err < 2e-2
    # a second launch on the same stream: the split tickets were left at zero
    again = llm.paged_verify(_rows(gq), gk, gv, gbt, gctx, gn, T, H, Hkv)
    torch.cuda.synchronize()
    assert torch.equal(again, got)


@pytest.mark.parametrize("splits", [(1, 1), (2, 1), (32, 1)], ids=["1split", "2splits", "32splits"])
def test_split_counts_the_policy_does_not_pick(splits):
    """The launch's split policy gives this batch 9 splits of 4 blocks, one block per wave.  One and
    two splits make the waves of the 2100-token sequence loop over their blocks (9 and 5 each); 32
    leaves most splits of every sequence without blocks."""
    H, Hkv, D, T = 14, 2, 64, 4
    case = _case(H, Hkv, D, T, torch.bfloat16, seed=11)
    qbuf, kc, vc, bt, ctx, n_rows = case
    ref = llm.paged_verify(_rows(qbuf), kc, vc, bt.clamp(max=kc.shape[0] - 1), ctx, n_rows, T, H, Hkv)
    gq, gk, gv, gbt, gctx, gn = _gpu(case)
    got = llm.paged_verify(_rows(gq), gk, gv, gbt, gctx, gn, T, H, Hkv, splits=splits)
    torch.cuda.synchronize()
    err = _rel(got, ref)
    print(f"paged_verify splits={splits}: rel err {err:.3e}")
    assert torch.isfinite(got.float()).all() and err < 2e-2


@pytest.mark.parametrize("dtype", [torch.bfloat16, FP8], ids=["bf16", "fp8"])
@pytest.mark.parametrize("H,Hkv,D", SHAPES)
def test_one_row_equals_paged_decode(H, Hkv, D, dtype):
    gq, gk, gv, gbt, gctx, gn = _gpu(_case(H, Hkv, D, 1, dtype, seed=7))
    got = llm.paged_verify(_rows(gq), gk, gv, gbt, gctx, gn, 1, H, Hkv)
    dec = llm.paged_decode(_rows(gq), gk, gv, gbt.clamp(max=gk.shape[0] - 1), gctx, H, Hkv)
    torch.cuda.synchronize()
    assert torch.isfinite(dec.float()).all()
    err = _rel(got, dec)
    print(f"paged_verify T=1 vs paged_decode H={H} D={D} {dtype}: rel err {err:.3e}")
    assert err < 2e-2


@pytest.mark.parametrize("dtype", [torch.bfloat16, FP8], ids=["bf16", "fp8"])
def test_each_row_equals_a_truncated_decode(dtype):
    """Row i of a T = 4 launch is one decode sequence of the same block list with ctx_len cut to
    that row's position + 1."""
    H, Hkv, D, T = 14, 2, 64, 4
    gq, gk, gv, gbt, gctx, gn = _gpu(_case(H, Hkv, D, T, dtype, seed=9))
    got = llm.paged_verify(_rows(gq), gk, gv, gbt, gctx, gn, T, H, Hkv)
    B = gctx.numel()
    live = (torch.arange(T, device=DEV)[None, :] < gn[:, None]).reshape(-1)              # [B*T]
    dctx = (gctx[:, None] - gn[:, None] + 1 + torch.arange(T, device=DEV)[None, :]).reshape(-1)
    dctx = torch.where(live, dctx, torch.ones_like(dctx)).int()
    dbt = gbt.clamp(max=gk.shape[0] - 1).repeat_interleave(T, 0).contiguous()
    dec = llm.paged_decode(_rows(gq), gk, gv, dbt, dctx, H, Hkv)
    torch.cuda.synchronize()
    assert live.sum() == int(gn.sum()) and B * T == live.numel()
    err = _rel(got[live], dec[live])
    print(f"paged_verify rows vs truncated paged_decode {dtype}: rel err {err:.3e}")
    assert torch.isfinite(dec[live].float()).all() and err < 2e-2


def test_paged_verify_rejects_bad_arguments():
    H, Hkv, D, T = 4, 4, 64, 4
    gq, gk, gv, gbt, gctx, gn = _gpu(_case(H, Hkv, D, T, torch.bfloat16, seed=1, first_pos=(1, 62)))
    q = _rows(gq)
    with pytest.raises(ValueError, match="columns"):
        llm.paged_verify(q, gk, gv, gbt, gctx, gn, 65, H, Hkv)
    with pytest.raises(ValueError, match="B\\*T"):
        llm.paged_verify(q[:-1], gk, gv, gbt, gctx, gn, T, H, Hkv)
    with pytest.raises(ValueError, match="match"):
        llm.paged_verify(q, gk, gv, gbt, gctx[:-1], gn, T, H, Hkv)
    with pytest.raises(ValueError, match="out"):
        llm.paged_verify(q, gk, gv, gbt, gctx, gn, T, H, Hkv, out=torch.empty(3, H * D, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(RuntimeError, match="n_rows int32"):
        llm.paged_verify(q, gk, gv, gbt, gctx, gn.long(), T, H, Hkv)
    with pytest.raises(RuntimeError, match="block_table int32"):
        llm.paged_verify(q, gk, gv, gbt.long(), gctx, gn, T, H, Hkv)
    with pytest.raises(RuntimeError):
        llm.paged_verify(q, gk, gv.to(FP8), gbt, gctx, gn, T, H, Hkv)
    with pytest.raises(ValueError, match="16 query heads"):
        llm.paged_verify(q, gk[:, :1], gv[:, :1], gbt, gctx, gn, 1, 17, 1)
