"""Pooled final block (models/clip.py::_pooled_final_block) on the CPU in fp32: the block's output at the
pooled rows must equal the last block of run_blocks there, in the plain form (K / V of all rows, one
query row) and in the fold form the GPU runs (query pushed through the LN-folded K weights, softmax-
weighted sum of the raw rows through the folded V weights: ops.pooled_attention_x)."""
import shutil
import subprocess
import re
from pathlib import Path

import pytest
import torch

import lumen_amd.models.clip as clip_mod
from lumen_amd import ops
from lumen_amd.models.clip import CLIPModel, _pooled_final_block, run_blocks


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-6)).item()


def _tower_inputs(tower, B, S, seed):
    """A residual stream with per-row means and scales that differ (the fold's row terms matter), and
    non-trivial LayerNorm parameters and biases (the K bias / LN beta constants must cancel)."""
    g = torch.Generator().manual_seed(seed)
    W = tower.cfg.width
    with torch.no_grad():     # in-place on the parameters themselves: bumps the versions _Block.lnf() keys on
        for blk in tower.blocks:
            for p in (blk.ln1_w, blk.ln2_w):
                p.copy_(1.0 + 0.3 * torch.randn(W, generator=g))
            for p in (blk.ln1_b, blk.ln2_b, blk.qkv_b, blk.out_b, blk.fc1_b, blk.fc2_b):
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
    x = torch.randn(B * S, W, generator=g) * (0.5 + 2.0 * torch.rand(B * S, 1, generator=g))
    return x + 3.0 * torch.randn(B * S, 1, generator=g)


@pytest.fixture(scope="module")
def tiny():
    return CLIPModel.random("tiny", seed=11, dtype=torch.float32)


@pytest.mark.parametrize("fold", [False, True])
def test_pooled_block_matches_last_block_vision(tiny, fold):
    t = tiny.visual
    cfg, B, S = t.cfg, 3, t.seq
    x = _tower_inputs(t, B, S, 1)
    ref = run_blocks(x.clone(), t.blocks[-1:], B, S, cfg.heads, cfg.act, cfg.ln_eps).view(B, S, -1)[:, 0]
    x0 = x.clone()
    got = _pooled_final_block(x, t.blocks[-1], B, S, cfg.heads, cfg.act, cfg.ln_eps, fold=fold)
    assert torch.equal(x, x0), "the residual stream must be left as it was"
    assert got.shape == ref.shape and _rel(got, ref) < 1e-4


@pytest.mark.parametrize("fold", [False, True])
def test_pooled_block_matches_last_block_text(tiny, fold):
    t = tiny.text
    cfg, S = t.cfg, t.cfg.context_length
    eot = torch.tensor([0, S // 2, S - 1])
    B = eot.numel()
    x = _tower_inputs(t, B, S, 2)
    full = run_blocks(x.clone(), t.blocks[-1:], B, S, cfg.heads, cfg.act, cfg.ln_eps, causal=True).view(B, S, -1)
    ref = full[torch.arange(B), eot]
    got = _pooled_final_block(x, t.blocks[-1], B, S, cfg.heads, cfg.act, cfg.ln_eps, q_rows=eot,
                              kv_len=(eot + 1).to(torch.int32), fold=fold)
    assert _rel(got, ref) < 1e-4


def test_fold_form_agrees_with_plain_form(tiny):
    """Fold-form reference built from g, s, z and c in fp32 against the plain attention output."""
    t = tiny.text
    cfg, S, W, H = t.cfg, t.cfg.context_length, t.cfg.width, t.cfg.heads
    D = W // H
    eot = torch.tensor([0, 5, S - 1, 9])
    B = eot.numel()
    x = _tower_inputs(t, B, S, 3)
    blk = t.blocks[-1]
    rows = torch.arange(B) * S + eot
    # plain: attention of the pooled rows over K / V of all rows
    h = ops.layer_norm(x, blk.ln1_w, blk.ln1_b, cfg.ln_eps)
    qkv = ops.linear(h, blk.qkv_w, blk.qkv_b)
    q5 = qkv.view(B, S, 3, H, D)
    q = qkv[rows, :W].reshape(B, 1, H, D)
    plain = ops.attention(q, q5[:, :, 1], q5[:, :, 2], kv_len=(eot + 1).int()).reshape(B, W)
    # fold: g = scale * q_h . Wk'_h, s = its row sums, (z, c) over the raw rows, then the folded V weights
    qw, qa = ops.ln_fold_weights(blk.qkv_w, blk.qkv_b, blk.ln1_w, blk.ln1_b)
    st = ops.ln_row_stats(x, cfg.ln_eps)
    g = torch.einsum("bhd,hdw->bhw", q.view(B, H, D), qw[W:2 * W].view(H, D, W)) * D ** -0.5
    z, c = ops.pooled_attention_x(x, st, g, g.sum(-1), S, (eot + 1).int())
    v = z @ qw[2 * W:].t() + c[:, None] * qa[0, 2 * W:] + qa[1, 2 * W:]
    hd = torch.arange(H)
    fold = v.view(B, H, H, D)[:, hd, hd].reshape(B, W)
    assert _rel(fold, plain) < 1e-4


def test_towers_with_and_without_pooled_final(tiny, monkeypatch):
    imgs = torch.randint(0, 256, (3, 40, 36, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    ids = torch.randint(1, 400, (3, tiny.cfg.text.context_length), generator=torch.Generator().manual_seed(1))
    ids[0, 0] = ids[1, 7] = ids[2, -1] = tiny.cfg.text.vocab_size - 1
    monkeypatch.setattr(clip_mod, "_POOLED_FINAL", False)
    e0, t0 = tiny.encode_image_uint8(imgs), tiny.encode_text_ids(ids)
    monkeypatch.setattr(clip_mod, "_POOLED_FINAL", True)
    e1, t1 = tiny.encode_image_uint8(imgs), tiny.encode_text_ids(ids)
    assert (e0 * e1).sum(-1).min().item() > 1 - 1e-5
    assert (t0 * t1).sum(-1).min().item() > 1 - 1e-5


def test_one_block_tower_runs_pooled_block_alone():
    cfg = clip_mod.CLIPConfig(embed_dim=64,
                              vision=clip_mod.VisionConfig(image_size=32, patch_size=8, width=64, layers=1, heads=2),
                              text=clip_mod.TextConfig(context_length=16, vocab_size=512, width=64, layers=1, heads=2))
    m = CLIPModel.random(cfg, seed=2, dtype=torch.float32)
    imgs = torch.randint(0, 256, (2, 32, 32, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    e1 = m.encode_image_uint8(imgs)
    clip_mod._POOLED_FINAL = False
    try:
        e0 = m.encode_image_uint8(imgs)
    finally:
        clip_mod._POOLED_FINAL = True
    assert (e0 * e1).sum(-1).min().item() > 1 - 1e-5


def test_shapes_the_kernel_does_not_take_fall_back():
    assert ops.pooled_attention_ok(1024, 16, 257) and ops.pooled_attention_ok(768, 12, 77)
    assert ops.pooled_attention_ok(64, 2, 17) and ops.pooled_attention_ok(1280, 10, 257)
    assert not ops.pooled_attention_ok(96, 3, 17)        # W % 64
    assert not ops.pooled_attention_ok(1024, 64, 257)    # head dim 16
    assert not ops.pooled_attention_ok(1024, 16, 1025)   # S > 1024
    assert not ops.pooled_attention_ok(1088, 17, 257)    # 17 waves of 64 columns


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")
def test_pooled_attention_kernel_does_not_spill():
    """The no-spill guard of tests/test_kernel_resources.py for csrc/pooled_attn.hip (ScratchSize only)."""
    src = Path(__file__).resolve().parents[1] / "lumen_amd" / "csrc" / "pooled_attn.hip"
    out = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", str(src),
                          "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    assert names, "no kernels reported"
    bad = [(n, s) for n, s in zip(names, scratch) if s > 0]
    assert not bad, f"kernels with scratch spills: {bad}"
