"""Pooled final block on the GPU: ops.pooled_attention_x (csrc/pooled_attn.hip) against its CPU reference, and
the CLIP towers with models.clip._POOLED_FINAL on and off against the CPU fp32 model."""
import functools

import pytest
import torch

import lumen_amd.models.clip as clip_mod
from lumen_amd import ops
from lumen_amd.models.clip import CLIPConfig, CLIPModel, TextConfig, VisionConfig

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-6)).item()


# (B, S, W, H, kv_len)
CASES = [
    (1, 17, 64, 2, None),         # the tiny geometry: head count below the MFMA M, one wave
    (3, 257, 256, 4, None),       # ragged 257 tail, odd batch
    (2, 77, 512, 8, [1, 77]),     # one-key softmax and full length
    (2, 197, 768, 12, None),      # 12 heads, 128-column waves
    (2, 64, 1024, 16, None),      # exactly four 16-token chunks, no ragged tail
]


def _op_inputs(B, S, W, H, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B * S, W, generator=g) * 3 + 5).to(torch.bfloat16)     # large mean: the st[j, 1] * s term matters
    st = ops.ln_row_stats(x.float(), 1e-5)
    gq = (torch.randn(B, H, W, generator=g) * W ** -0.5).to(torch.bfloat16)  # scores of unit spread
    return x, st, gq, gq.float().sum(-1)


@pytest.mark.parametrize("B,S,W,H,kv", CASES)
def test_pooled_attention_x_matches_cpu(B, S, W, H, kv):
    x, st, g, s = _op_inputs(B, S, W, H, 7)
    kl = torch.tensor(kv, dtype=torch.int32) if kv is not None else None
    z_ref, c_ref = ops.pooled_attention_x(x.float(), st, g.float(), s, S, kl)
    z, c = ops.pooled_attention_x(x.to(DEV), st.to(DEV), g.to(DEV), s.to(DEV), S, kl.to(DEV) if kl is not None else None)
    torch.cuda.synchronize()
    assert z.shape == (B * H, W) and z.dtype == torch.bfloat16 and c.shape == (B * H,)
    ez, ec = _rel(z, z_ref), _rel(c, c_ref)
    print(f"pooled_attention_x B={B} S={S} W={W} H={H}: rel z {ez:.2e} c {ec:.2e}")
    assert ez < 2e-2 and ec < 2e-2


def test_pooled_attention_x_one_hot_token():
    """A huge score on ONE token per (sequence, head), a different one for each: z must be that token's
    rstd * x_j and c its st[j, 1].  z = bf16(bf16(rstd) . x_j): two bf16 roundings of 2^-8 each."""
    B, S, W, H = 2, 257, 256, 4
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(B * S, W, generator=gen).to(torch.bfloat16)
    st = ops.ln_row_stats(x.float(), 1e-5)
    tok = torch.tensor([[(67 * h + 3 * b + 1) % S for h in range(H)] for b in range(B)])
    tok[1, 3] = S - 1                                     # the ragged last chunk's only token
    rows = (torch.arange(B)[:, None] * S + tok).reshape(-1)
    g = x[rows].view(B, H, W)                             # score of the chosen token ~ W, of the others ~ sqrt(W)
    z, c = ops.pooled_attention_x(x.to(DEV), st.to(DEV), g.to(DEV).contiguous(), g.float().sum(-1).to(DEV), S)
    torch.cuda.synchronize()
    z_ref = st[rows, :1] * x[rows].float()
    assert torch.allclose(z.float().cpu(), z_ref, rtol=2.0 ** -7 * 1.01, atol=1e-30)
    assert torch.allclose(c.cpu(), st[rows, 1], rtol=1e-5, atol=1e-6)


MID = CLIPConfig(embed_dim=64, vision=VisionConfig(image_size=56, patch_size=14, width=256, layers=3, heads=4),
                 text=TextConfig(context_length=24, vocab_size=512, width=256, layers=3, heads=4))


@functools.lru_cache(maxsize=None)
def _models_and_refs(name):
    cfg = clip_mod.PRESETS["tiny"] if name == "tiny" else MID
    m_cpu = CLIPModel.random(cfg, seed=9, dtype=torch.float32)
    m_gpu = CLIPModel.random(cfg, seed=9, dtype=torch.bfloat16, device=DEV)
    s, ctx = cfg.vision.image_size, cfg.text.context_length
    gen = torch.Generator().manual_seed(5)
    imgs = torch.randint(0, 256, (5, s + 9, s + 4, 3), dtype=torch.uint8, generator=gen)
    ids = torch.randint(1, 400, (5, ctx), generator=gen)
    for b, e in enumerate([0, 5, ctx - 1, ctx // 2, 1]):      # EOT = the max id, first / middle / last positions
        ids[b, e] = cfg.text.vocab_size - 1
    return m_gpu, imgs, ids, m_cpu.encode_image_uint8(imgs), m_cpu.encode_text_ids(ids)


@pytest.mark.parametrize("micro", [False, True])
@pytest.mark.parametrize("name", ["tiny", "mid"])
def test_towers_pooled_final_on_off(monkeypatch, name, micro):
    m, imgs, ids, e_ref, t_ref = _models_and_refs(name)
    # micro: batches of 5 cut 2 + 3 over two streams; otherwise far below the micro-batch row threshold
    monkeypatch.setattr(clip_mod, "_VIT_MICRO_MIN_ROWS", 0 if micro else 1 << 30)
    monkeypatch.setattr(clip_mod, "_TEXT_MICRO_MIN_ROWS", 0 if micro else 1 << 30)
    monkeypatch.setattr(clip_mod, "_POOLED_FINAL_MIN_ROWS", 0)      # these batches are far below the row threshold
    calls = []
    real = ops.pooled_attention_x
    monkeypatch.setattr(ops, "pooled_attention_x", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    out = {}
    for on in (False, True):
        monkeypatch.setattr(clip_mod, "_POOLED_FINAL", on)
        out[on] = (m.encode_image_uint8(imgs.to(DEV)).cpu(), m.encode_text_ids(ids.to(DEV)).cpu())
        assert len(calls) == (2 if on else 0), "the pooled block must run for both towers when on, never when off"
    torch.cuda.synchronize()
    for on in (False, True):
        e, t = out[on]
        ce, ct = (e * e_ref).sum(-1).min().item(), (t * t_ref).sum(-1).min().item()
        print(f"{name} micro={micro} pooled={on}: min cos vs CPU image {ce:.5f} text {ct:.5f}")
        assert ce > 0.995 and ct > 0.995
    assert (out[True][0] * out[False][0]).sum(-1).min().item() > 0.995
    assert (out[True][1] * out[False][1]).sum(-1).min().item() > 0.995
