"""Paged-prefill attention kernel (csrc/llm.hip: new query rows over the paged KV pools) vs the
fp32 CPU reference, vs the paged-decode kernel, and through chunked LLM.prefill vs the gather path."""
import numpy as np
import pytest
import torch

from lumen_amd.models.llm import LLM, LLM_PRESETS
from lumen_amd.ops import llm
from lumen_amd.runtime.kv_cache import PagedKVCache

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-6)).item()


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.float().flatten(), b.float().flatten(), dim=0).item()


def _case(H, Hkv, D, start, T, dtype, seed):
    """CPU tensors: packed QKV rows (a strided view), the two pools with every slot that is not one
    of the sequence's start + T tokens set to NaN (bf16 0x7FC0 / e4m3fn 0x7F), the shuffled block list."""
    g = torch.Generator().manual_seed(seed)
    S = start + T
    nb = -(-S // 64)
    NB = nb + 3                                              # spare pool blocks, all NaN
    blocks = torch.randperm(NB, generator=g)[:nb].long()
    raw, nan = (torch.uint8, 0x7F) if dtype == FP8 else (torch.int16, 0x7FC0)
    pools = []
    for transposed in (False, True):
        vals = torch.randn(S, Hkv, D, generator=g).to(dtype).view(raw)
        full = torch.full((nb * 64, Hkv, D), nan, dtype=raw)
        full[:S] = vals
        full = full.view(nb, 64, Hkv, D)
        pool = torch.full((NB, Hkv, D, 64) if transposed else (NB, Hkv, 64, D), nan, dtype=raw)
        pool[blocks] = full.permute(0, 2, 3, 1) if transposed else full.permute(0, 2, 1, 3)
        pools.append(pool.view(dtype))
    # 8 spare columns per row: _rows() cuts them off again, on the device the buffer ends up on
    qbuf = torch.randn(T, (H + 2 * Hkv) * D + 8, generator=g).bfloat16()
    return qbuf, pools[0], pools[1], blocks


def _rows(qbuf):
    """the packed QKV rows as a view whose row stride is not its width"""
    q = qbuf[:, :qbuf.shape[1] - 8]
    assert q.stride(0) == q.shape[1] + 8 and q.data_ptr() == qbuf.data_ptr()
    return q


@pytest.mark.parametrize("dtype", [torch.bfloat16, FP8], ids=["bf16", "fp8"])
@pytest.mark.parametrize("start,T", [(0, 70), (64, 1), (64, 17), (100, 130), (577, 47)])
@pytest.mark.parametrize("H,Hkv,D", [(14, 2, 64), (32, 8, 128), (4, 4, 64), (16, 1, 64), (4, 2, 32)])
def test_paged_prefill_vs_cpu_reference(H, Hkv, D, start, T, dtype):
    qbuf, kc, vc, blocks = _case(H, Hkv, D, start, T, dtype, seed=H * D + start + T)
    assert not torch.isfinite(kc.float()).all() and not torch.isfinite(vc.float()).all()   # the NaN slots are there
    ref = llm.paged_prefill(_rows(qbuf), kc, vc, blocks, start, H, Hkv)       # fp32 math on the dequantised cache
    assert ref.shape == (T, H * D) and torch.isfinite(ref.float()).all(), "the reference must not see the NaN slots"
    guard = torch.full((T + 2, H * D), 777.0, dtype=torch.bfloat16, device=DEV)
    out = guard[1:T + 1]
    got = llm.paged_prefill(_rows(qbuf.to(DEV)), kc.to(DEV), vc.to(DEV), blocks.to(DEV), start, H, Hkv, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.isfinite(got.float()).all()
    assert (guard[0] == 777.0).all() and (guard[T + 1] == 777.0).all(), "guard rows overwritten"
    err = _rel(got, ref)
    print(f"paged_prefill H={H} Hkv={Hkv} D={D} start={start} T={T} {dtype}: rel err {err:.3e}")
    assert err < 2e-2


@pytest.mark.parametrize("dtype", [torch.bfloat16, FP8], ids=["bf16", "fp8"])
def test_paged_prefill_matches_paged_decode(dtype):
    """Every query row is one decode sequence of the same block list with ctx_len = start + i + 1."""
    H, Hkv, D, start, T = 14, 2, 64, 100, 130
    qbuf, kc, vc, blocks = (t.to(DEV) for t in _case(H, Hkv, D, start, T, dtype, seed=3))
    qkv = _rows(qbuf)
    got = llm.paged_prefill(qkv, kc, vc, blocks, start, H, Hkv)
    bt = blocks.int()[None, :].repeat(T, 1).contiguous()
    ctx = (start + 1 + torch.arange(T, device=DEV)).int()
    dec = llm.paged_decode(qkv, kc, vc, bt, ctx, H, Hkv)
    torch.cuda.synchronize()
    assert torch.isfinite(dec.float()).all()
    err = _rel(got, dec)
    print(f"paged_prefill vs paged_decode {dtype}: rel err {err:.3e}")
    assert err < 2e-2


def test_paged_prefill_rejects_bad_arguments():
    H, Hkv, D = 4, 4, 64
    qbuf, kc, vc, blocks = (t.to(DEV) for t in _case(H, Hkv, D, 64, 17, torch.bfloat16, seed=1))
    qkv = _rows(qbuf)
    with pytest.raises(RuntimeError, match="block list"):
        llm.paged_prefill(qkv, kc, vc, blocks[:1], 64, H, Hkv)
    with pytest.raises(RuntimeError, match="out rows"):
        llm.paged_prefill(qkv, kc, vc, blocks, 64, H, Hkv, out=torch.empty(3, H * D, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(RuntimeError, match="blocks int64"):
        llm.paged_prefill(qkv, kc, vc, blocks.int(), 64, H, Hkv)
    with pytest.raises(RuntimeError):
        llm.paged_prefill(qkv, kc, vc.to(FP8), blocks, 64, H, Hkv)


def test_chunked_prefill_runs_the_kernel_and_matches_the_gather_path(monkeypatch):
    """Qwen2-0.5B, 700 tokens in 128-token chunks: LLM.prefill on the paged-prefill kernel vs the
    gather path (LUMEN_PAGED_PREFILL=0), logits and a layer's K cache."""
    cfg = LLM_PRESETS["qwen2-0.5b"]
    m = LLM(cfg, device=DEV)
    m.random_init(4)
    ids = torch.tensor(np.random.default_rng(20).integers(0, 150000, 700), device=DEV)
    calls = []
    real = llm.paged_prefill

    def spy(*a, **k):
        calls.append(a[4])          # start_pos
        return real(*a, **k)

    monkeypatch.setattr(llm, "paged_prefill", spy)
    res, ncalls = {}, {}
    for knob in ("1", "0"):
        monkeypatch.setenv("LUMEN_PAGED_PREFILL", knob)
        calls.clear()
        kv = PagedKVCache(cfg.num_layers, m.Hkv, cfg.head_dim, num_blocks=32, device=DEV)
        assert kv.blocks.reserve(1, 700)
        x = m.embed_tokens(ids)
        tab = torch.from_numpy(np.asarray(kv.blocks.table(1), np.int64)).cuda()
        for s in range(0, 700, 128):
            e = min(700, s + 128)
            slots = torch.from_numpy(kv.slots(1, s, e - s)).cuda()
            logits = m.prefill(x[s:e], kv, slots, start_pos=s, prefix_blocks=tab[: -(-e // 64)] if s else None)
        res[knob] = (logits.float(), kv.k[5][tab].float(), kv.v[5][tab].float())
        ncalls[knob] = list(calls)
    # every chunk after the first, every layer, went through the kernel -- and none with the knob off
    assert sorted(set(ncalls["1"])) == [128, 256, 384, 512, 640] and len(ncalls["1"]) == 5 * cfg.num_layers
    assert ncalls["0"] == []
    for a, b in zip(res["1"], res["0"]):
        assert torch.isfinite(a).all()
        assert _cos(a, b) > 0.999


def test_chunk_row_threshold_between_kernel_and_gather_path(monkeypatch):
    """Chunks of up to _PAGED_PREFILL_MAX_ROWS rows run on the kernel, larger ones on the gather path
    (measured crossover, profiles/prefix_cache_kernel_v1.txt); both sides of the threshold agree with
    the gather path on the same rows."""
    from lumen_amd.models import llm as mllm

    cfg = LLM_PRESETS["qwen2-0.5b"]
    m = LLM(cfg, device=DEV)
    m.random_init(7)
    R = mllm._PAGED_PREFILL_MAX_ROWS
    ids = torch.tensor(np.random.default_rng(2).integers(0, 150000, 64 + R + 1), device=DEV)
    calls = []
    real = llm.paged_prefill

    def spy(*a, **k):
        calls.append(a[0].shape[0])
        return real(*a, **k)

    monkeypatch.setattr(llm, "paged_prefill", spy)
    out = {}
    for T in (R, R + 1):
        for knob in ("1", "0"):
            monkeypatch.setenv("LUMEN_PAGED_PREFILL", knob)
            calls.clear()
            kv = PagedKVCache(cfg.num_layers, m.Hkv, cfg.head_dim, num_blocks=16, device=DEV)
            assert kv.blocks.reserve(1, 64 + T)
            x = m.embed_tokens(ids[:64 + T])
            tab = torch.from_numpy(np.asarray(kv.blocks.table(1), np.int64)).cuda()
            m.prefill(x[:64], kv, torch.from_numpy(kv.slots(1, 0, 64)).cuda())
            out[T, knob] = m.prefill(x[64:], kv, torch.from_numpy(kv.slots(1, 64, T)).cuda(), start_pos=64,
                                     prefix_blocks=tab).float()
            assert calls == ([T] * cfg.num_layers if knob == "1" and T <= R else [])
        assert torch.isfinite(out[T, "1"]).all() and _cos(out[T, "1"], out[T, "0"]) > 0.999
