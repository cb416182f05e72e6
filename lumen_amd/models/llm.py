"""Llama / Qwen2 / Qwen3 / Qwen3-MoE / Qwen-VL decoder for the VLM, tensor-parallel over RCCL.

Reference: the FastVLM decoder ONNX graph (Qwen2-0.5B) driven by
packages/lumen-vlm/src/lumen_vlm/backends/onnxrt_backend.py:161-533; the north star
adds Llama-3-8B (LLaVA-style) at TP=8.  Per layer (every op one gfx950 kernel):

  RMSNorm (fused residual add)  ->  QKV GEMM (+bias, Qwen2)  ->  RoPE + paged-KV write
  (Qwen3: q and k heads first pass through an RMSNorm over head_dim, inside the same kernel;
  its decode steps keep this launch, since the attention kernel's fused RoPE has no norm)
  ->  attention (prefill: flash kernel reading the rotated QKV in place, causal;
      decode: paged flash-decoding)  ->  o_proj GEMM  ->  RMSNorm  ->  gate|up GEMM with
  the SwiGLU epilogue  ->  down GEMM

Qwen3-MoE (``num_experts > 0``): the MLP of every layer is sparse -- RMSNorm -> router (fp32
logits, top-k, ties to the lower id) -> the chosen experts' gate|up + SwiGLU and down GEMMs over
rows grouped by expert on the device -> weighted combine into the residual stream
(``ops.llm.moe_mlp``, csrc/moe.hip).  No host read and launches sized from the shapes alone, so
decode and verify steps are captured into graphs like the dense ones.  Such a decoder runs the
unfolded layer stack at every row count.  Quantised experts are an explicit opt-in,
``quantize_fp8(experts=True)`` / ``quantize_w4(experts=True)``: weight-only in both formats (fp8
or 4-bit codes into bf16 MFMAs, csrc/moe_wq.hip), the router stays in the activation dtype;
without the opt-in the two methods refuse a MoE decoder.  Out of scope and refused with an error:
tensor / expert parallelism (``tp.world > 1``), the norm-folded decode chain (``fold_norms`` leaves
it unfolded) and mixed dense / sparse stacks (``decoder_sparse_step != 1``, ``mlp_only_layers``).

Qwen2-VL / Qwen2.5-VL / Qwen3-VL decoders (``rope_scaling`` with ``mrope_section``): multimodal RoPE.
Every token has three positions (temporal, height, width; ``ops.llm.mrope_positions``) and each
rotary frequency takes its angle from one of them (``LLMConfig.mrope``, ``ops.llm.mrope_axes``).  Only
the prefill needs the three axes (``prefill(pos3=...)``, the MROPE form of the RoPE kernels): a
generated token is a text token whose three positions are equal, cache index + the prompt's rope
delta, so ``decode`` / ``verify`` run the 1-D kernels at that shifted position.  The causal masks
keep using cache indices.  Their checkpoints hold the decoder under ``model.language_model.``
(``load_hf_state_dict(prefix=...)``).  Out of scope: the Qwen-VL vision towers, DeepStack inputs,
video grids, tensor parallelism with ``pos3`` and the fused experts of Qwen3-VL-MoE (refused).

Tensor parallelism (Megatron): QKV and gate|up are column-parallel (whole heads /
whole 8-column GLU groups per rank), o_proj and down are row-parallel followed by
an all-reduce (RCCL); with TP the residual add is fused into the next RMSNorm
(``norm(add=partial, resid_out=x)``) instead of the GEMM epilogue.  Embedding and
lm_head are vocab-parallel (masked lookup + all-reduce; local top-k + all-gather of
the candidates for sampling).  The Qwen3 q / k norm weights ([head_dim], shared by all heads)
are replicated on every rank.  Weights can be loaded from HF Qwen2/Qwen3/Llama state dicts
(sharded at load) or random-initialised per rank directly on the device.
"""
from __future__ import annotations


import math
import os
from dataclasses import asdict, dataclass, field
from typing import Optional, Sequence

import numpy as np
import torch
from torch import nn

from .. import ops
from ..ops import llm as lops

# Every projection runs on the hand-written kernels: bf16 prefill on the MFMA GEMMs (128x128
# LDS-DMA pipeline at a few hundred tokens), fp8 prefill W8A8 on the fp8 matrix cores
# (ops.linear_f8, csrc/gemm_f8.hip, per-token scales from the fused RMSNorm+quant kernel),
# decode on the skinny split-K kernels.  The r1 hipBLASLt prefill path is gone: FastVLM-0.5B
# TTFT measured 12.25-12.72 ms without it vs 12.60-12.76 ms with it (same box, r2).
# W8A8 prefill from this many tokens up (decode batches stay on the weight-only skinny kernels)
_F8_MIN_ROWS = 33
# GPU: RMSNorm gammas folded into qkv / gate|up / lm_head (LLM.fold_norms); decode norms become
# rstd row scales in the skinny GEMM epilogues (ops.linear_dec)
_FUSED_DECODE_NORM = True
# decode: RoPE + current-token KV-cache write inside the paged attention kernel (no rope_kv launch)
_FUSED_DECODE_ROPE = True
# TP prefill from this many rows up: the rows run as two halves whose row-parallel all-reduces go
# to a communication stream, so half A's all-reduce overlaps half B's GEMMs (624-token
# LLaVA prompts at TP 8: 64 x 5 MB all-reduces on the time-to-first-token path)
_TP_OVERLAP_MIN_ROWS = 256
# chunked prefill / prefix reuse (start_pos > 0): chunks of up to this many rows attend the paged
# cache through the paged-prefill kernel (csrc/llm.hip).  Larger chunks, and LUMEN_PAGED_PREFILL=0,
# gather the prefix out of the pools and run the flash kernel on the copy: at the Llama-3-8B layer
# shape the kernel takes 0.55-0.89x the gather path's time up to 512 rows (contexts to 8k, bf16 and
# fp8 caches) but 1.06-1.9x from 1024 rows up, where its workgroups (one per CU at a time: the K / V
# fragments of a block fill the register file) no longer fit one round over the 256 CUs
# (profiles/prefix_cache_kernel_v1.txt)
_PAGED_PREFILL_MAX_ROWS = 512
# (r4's fused MX prefill chain -- block-scaled activations from the epilogues, 6 launches per
# layer -- lost its A/B to this per-token chain, 13.12 vs 12.79 ms TTFT, profiles/r4_mx_chain_ab_v1.txt,
# and was removed in r5; the MX W8A8 chain stays for the ViT tower, models/clip.py:run_blocks_mx)


# HF model types by decoder family; the Qwen-VL ones also come as the ``text_config`` of a VLM config
_QWEN_VL_TYPES = ("qwen2_vl", "qwen2_5_vl", "qwen3_vl", "qwen2_vl_text", "qwen2_5_vl_text", "qwen3_vl_text")
_QWEN2_TYPES = ("qwen2", "qwen2_vl", "qwen2_5_vl", "qwen2_vl_text", "qwen2_5_vl_text")          # qkv bias
_QWEN3_TYPES = ("qwen3", "qwen3_moe", "qwen3_vl", "qwen3_vl_text")                              # q / k norm


@dataclass
class LLMConfig:
    vocab_size: int = 151936
    hidden_size: int = 896
    num_layers: int = 24
    num_heads: int = 14
    num_kv_heads: int = 2
    head_dim: int = 64
    intermediate_size: int = 4864
    rope_theta: float = 1000000.0
    rms_eps: float = 1e-6
    max_position: int = 32768
    tie_word_embeddings: bool = True
    qkv_bias: bool = True
    qk_norm: bool = False            # Qwen3: RMSNorm over head_dim on every q / k head before RoPE
    rope_scaling: Optional[dict] = None
    bos_token_id: int = 151643
    eos_token_id: int = 151645
    # Qwen3-MoE: every layer's MLP is num_experts small SwiGLU experts of which a router picks
    # num_experts_per_tok per token (0 experts: the dense MLP of intermediate_size)
    num_experts: int = 0
    num_experts_per_tok: int = 0
    moe_intermediate_size: int = 0
    norm_topk_prob: bool = True

    @staticmethod
    def from_dict(d: dict) -> "LLMConfig":
        keys = LLMConfig.__dataclass_fields__.keys()
        return LLMConfig(**{k: v for k, v in d.items() if k in keys})

    @property
    def mrope(self) -> Optional[tuple]:
        """``(sections, interleaved)`` of a multimodal-RoPE decoder (Qwen-VL: ``rope_scaling`` carries
        ``mrope_section``), validated against head_dim; None for 1-D RoPE."""
        sec = (self.rope_scaling or {}).get("mrope_section")
        if sec is None:
            return None
        interleaved = bool(self.rope_scaling.get("mrope_interleaved", False))
        lops.mrope_axes(self.head_dim, sec, interleaved)      # raises on sections that do not fit head_dim
        return tuple(int(s) for s in sec), interleaved

    @staticmethod
    def from_hf(c: dict) -> "LLMConfig":
        mt = c.get("model_type", "llama")
        if any(t.startswith("qwen3_vl_moe") for t in (mt, (c.get("text_config") or {}).get("model_type", ""))):
            raise ValueError("qwen3_vl_moe: its checkpoints fuse the experts' weights into one tensor per layer, "
                             "which needs a loader of its own; not supported")
        if c.get("text_config") and mt in _QWEN_VL_TYPES:
            c = c["text_config"]
            mt = c.get("model_type", mt)
        H = c["num_attention_heads"]
        hd = c.get("head_dim") or c["hidden_size"] // H
        # newer HF configs carry the scaling dict, rope_theta included, as ``rope_parameters``
        rope = c.get("rope_scaling") or c.get("rope_parameters")
        moe = {}
        if mt == "qwen3_moe":
            if c.get("decoder_sparse_step", 1) != 1:
                raise ValueError(f"qwen3_moe: decoder_sparse_step = {c.get('decoder_sparse_step')}; only stacks whose "
                                 "every layer is sparse (decoder_sparse_step 1) are supported")
            if c.get("mlp_only_layers"):
                raise ValueError(f"qwen3_moe: mlp_only_layers = {c.get('mlp_only_layers')}; mixed dense / sparse "
                                 "stacks are not supported")
            moe = dict(num_experts=c["num_experts"], num_experts_per_tok=c["num_experts_per_tok"],
                       moe_intermediate_size=c["moe_intermediate_size"],
                       norm_topk_prob=bool(c.get("norm_topk_prob", False)))
        return LLMConfig(vocab_size=c["vocab_size"], hidden_size=c["hidden_size"], num_layers=c["num_hidden_layers"],
                         num_heads=H, num_kv_heads=c.get("num_key_value_heads", H), head_dim=hd,
                         intermediate_size=c["intermediate_size"],
                         rope_theta=c.get("rope_theta") or (rope or {}).get("rope_theta", 10000.0),
                         rms_eps=c.get("rms_norm_eps", 1e-6), max_position=c.get("max_position_embeddings", 4096),
                         tie_word_embeddings=c.get("tie_word_embeddings", False),
                         qkv_bias=c.get("attention_bias", mt in _QWEN2_TYPES), qk_norm=mt in _QWEN3_TYPES,
                         rope_scaling=rope,
                         bos_token_id=c.get("bos_token_id") or 0,
                         eos_token_id=(c.get("eos_token_id")[0] if isinstance(c.get("eos_token_id"), list)
                                       else c.get("eos_token_id") or 0), **moe)

    def to_dict(self):
        return asdict(self)


LLM_PRESETS = {
    "qwen2-0.5b": LLMConfig(),
    "llama3-8b": LLMConfig(vocab_size=128256, hidden_size=4096, num_layers=32, num_heads=32, num_kv_heads=8,
                           head_dim=128, intermediate_size=14336, rope_theta=500000.0, rms_eps=1e-5,
                           max_position=8192, tie_word_embeddings=False, qkv_bias=False, bos_token_id=128000,
                           eos_token_id=128009),
    "vicuna-7b": LLMConfig(vocab_size=32000, hidden_size=4096, num_layers=32, num_heads=32, num_kv_heads=32,
                           head_dim=128, intermediate_size=11008, rope_theta=10000.0, rms_eps=1e-5,
                           max_position=4096, tie_word_embeddings=False, qkv_bias=False, bos_token_id=1,
                           eos_token_id=2),
    "qwen3-0.6b": LLMConfig(vocab_size=151936, hidden_size=1024, num_layers=28, num_heads=16, num_kv_heads=8,
                            head_dim=128, intermediate_size=3072, rope_theta=1000000.0, rms_eps=1e-6,
                            max_position=40960, tie_word_embeddings=True, qkv_bias=False, qk_norm=True),
    "qwen3-8b": LLMConfig(vocab_size=151936, hidden_size=4096, num_layers=36, num_heads=32, num_kv_heads=8,
                          head_dim=128, intermediate_size=12288, rope_theta=1000000.0, rms_eps=1e-6,
                          max_position=40960, tie_word_embeddings=False, qkv_bias=False, qk_norm=True),
    # Qwen3-30B-A3B: 128 experts of 768, 8 per token (~3 B active parameters per decode step)
    "qwen3-30b-a3b": LLMConfig(vocab_size=151936, hidden_size=2048, num_layers=48, num_heads=32, num_kv_heads=4,
                               head_dim=128, intermediate_size=6144, rope_theta=1000000.0, rms_eps=1e-6,
                               max_position=40960, tie_word_embeddings=False, qkv_bias=False, qk_norm=True,
                               num_experts=128, num_experts_per_tok=8, moe_intermediate_size=768,
                               norm_topk_prob=True),
    "tiny": LLMConfig(vocab_size=512, hidden_size=128, num_layers=2, num_heads=4, num_kv_heads=2, head_dim=32,
                      intermediate_size=256, max_position=2048, bos_token_id=1, eos_token_id=2),
    # Qwen3 test shape: q / k norms, head_dim 64 (the RoPE tile kernel's smallest) and heads x head_dim != hidden
    "tiny-qwen3": LLMConfig(vocab_size=512, hidden_size=128, num_layers=2, num_heads=4, num_kv_heads=2, head_dim=64,
                            intermediate_size=256, max_position=2048, qkv_bias=False, qk_norm=True, bos_token_id=1,
                            eos_token_id=2),
    # Qwen-VL test shapes (multimodal RoPE): the tiny shape with head_dim 64, contiguous sections, qkv
    # bias and no q / k norm (Qwen2-VL / Qwen2.5-VL); tiny-qwen3 with interleaved sections (Qwen3-VL)
    "tiny-qwen2vl": LLMConfig(vocab_size=512, hidden_size=128, num_layers=2, num_heads=4, num_kv_heads=2,
                              head_dim=64, intermediate_size=256, max_position=2048, bos_token_id=1, eos_token_id=2,
                              rope_scaling={"rope_type": "default", "mrope_section": [8, 12, 12]}),
    "tiny-qwen3vl": LLMConfig(vocab_size=512, hidden_size=128, num_layers=2, num_heads=4, num_kv_heads=2,
                              head_dim=64, intermediate_size=256, max_position=2048, qkv_bias=False, qk_norm=True,
                              bos_token_id=1, eos_token_id=2,
                              rope_scaling={"rope_type": "default", "mrope_section": [12, 10, 10],
                                            "mrope_interleaved": True}),
    # Qwen3-MoE test shape: tiny-qwen3 with 8 experts of 64, 2 per token
    "tiny-qwen3-moe": LLMConfig(vocab_size=512, hidden_size=128, num_layers=2, num_heads=4, num_kv_heads=2,
                                head_dim=64, intermediate_size=256, max_position=2048, qkv_bias=False, qk_norm=True,
                                bos_token_id=1, eos_token_id=2, num_experts=8, num_experts_per_tok=2,
                                moe_intermediate_size=64, norm_topk_prob=True),
    # TP = 4 / 8 test shapes: 8 query heads over 8 KV heads (one of each per rank at TP = 8) and over
    # 2 KV heads (GQA: every KV head replicated on TP / 2 ranks, the kv_rep > 1 load path)
    "tiny-h8": LLMConfig(vocab_size=512, hidden_size=256, num_layers=2, num_heads=8, num_kv_heads=8, head_dim=32,
                         intermediate_size=512, max_position=2048, bos_token_id=1, eos_token_id=2),
    "tiny-gqa8": LLMConfig(vocab_size=512, hidden_size=256, num_layers=2, num_heads=8, num_kv_heads=2, head_dim=32,
                           intermediate_size=512, max_position=2048, bos_token_id=1, eos_token_id=2),
}


@dataclass
class TPInfo:
    rank: int = 0
    world: int = 1
    group: object = None

    @property
    def enabled(self) -> bool:
        return self.world > 1


class DecoderLayer(nn.Module):
    def __init__(self, cfg: LLMConfig, tp: TPInfo, dtype, device):
        super().__init__()
        kw = dict(dtype=dtype, device=device)
        Hd, D = cfg.hidden_size, cfg.head_dim
        self.H = cfg.num_heads // tp.world
        self.Hkv = max(cfg.num_kv_heads // tp.world, 1)
        self.I = cfg.intermediate_size // tp.world
        self.ln1 = nn.Parameter(torch.ones(Hd, **kw), requires_grad=False)
        self.ln2 = nn.Parameter(torch.ones(Hd, **kw), requires_grad=False)
        self.qkv_w = nn.Parameter(torch.zeros((self.H + 2 * self.Hkv) * D, Hd, **kw), requires_grad=False)
        self.qkv_b = nn.Parameter(torch.zeros((self.H + 2 * self.Hkv) * D, dtype=torch.float32, device=device),
                                  requires_grad=False) if cfg.qkv_bias else None
        # Qwen3: RMSNorm weights over head_dim, shared by all q (k) heads, hence replicated under TP
        self.q_norm = nn.Parameter(torch.ones(D, dtype=torch.float32, device=device),
                                   requires_grad=False) if cfg.qk_norm else None
        self.k_norm = nn.Parameter(torch.ones(D, dtype=torch.float32, device=device),
                                   requires_grad=False) if cfg.qk_norm else None
        self.o_w = nn.Parameter(torch.zeros(Hd, self.H * D, **kw), requires_grad=False)
        self.E = cfg.num_experts
        if self.E > 0:
            # sparse MLP (ops.llm.moe_mlp): router [E, hidden], per expert gate|up interleaved as
            # ops.glu_interleave [E, 2I, hidden] and down [E, hidden, I], I = moe_intermediate_size
            self.I = cfg.moe_intermediate_size
            self.router_w = nn.Parameter(torch.zeros(self.E, Hd, **kw), requires_grad=False)
            self.gu_w = nn.Parameter(torch.zeros(self.E, 2 * self.I, Hd, **kw), requires_grad=False)
            self.down_w = nn.Parameter(torch.zeros(self.E, Hd, self.I, **kw), requires_grad=False)
        else:
            self.gu_w = nn.Parameter(torch.zeros(2 * self.I, Hd, **kw), requires_grad=False)
            self.down_w = nn.Parameter(torch.zeros(Hd, self.I, **kw), requires_grad=False)


class LLM(nn.Module):
    def __init__(self, cfg: LLMConfig, tp: Optional[TPInfo] = None, dtype=torch.bfloat16, device=None):
        super().__init__()
        self.cfg = cfg
        self.tp = tp or TPInfo()
        w = self.tp.world
        assert cfg.num_heads % w == 0 and (cfg.num_kv_heads % w == 0 or w % cfg.num_kv_heads == 0), "TP heads"
        assert cfg.intermediate_size % (8 * w) == 0 and cfg.vocab_size % w == 0, "TP shapes"
        self.moe = cfg.num_experts > 0
        if self.moe:
            if w > 1:
                raise NotImplementedError("a mixture-of-experts decoder (num_experts > 0) runs on one GPU: tensor / "
                                          "expert parallelism is not implemented")
            if not (1 <= cfg.num_experts_per_tok <= min(cfg.num_experts, 8) and cfg.num_experts <= 256):
                raise ValueError(f"MoE: num_experts <= 256 and 1 <= num_experts_per_tok <= min(num_experts, 8), got "
                                 f"{cfg.num_experts} / {cfg.num_experts_per_tok}")
            if cfg.hidden_size % 32 or cfg.moe_intermediate_size % 32 or cfg.moe_intermediate_size <= 0:
                raise ValueError("MoE: hidden_size and moe_intermediate_size must be multiples of 32")
        self.Vl = cfg.vocab_size // w
        self.v0 = self.tp.rank * self.Vl
        kw = dict(dtype=dtype, device=device)
        self.embed = nn.Parameter(torch.zeros(self.Vl, cfg.hidden_size, **kw), requires_grad=False)
        self.layers = nn.ModuleList([DecoderLayer(cfg, self.tp, dtype, device) for _ in range(cfg.num_layers)])
        self.norm = nn.Parameter(torch.ones(cfg.hidden_size, **kw), requires_grad=False)
        self.lm_head = None if cfg.tie_word_embeddings else nn.Parameter(torch.zeros(self.Vl, cfg.hidden_size, **kw),
                                                                         requires_grad=False)
        self.register_buffer("cos_sin", lops.rope_cos_sin(cfg.max_position, cfg.head_dim, cfg.rope_theta,
                                                          cfg.rope_scaling).to(device), persistent=False)
        self.H, self.Hkv = self.layers[0].H, self.layers[0].Hkv
        self.comm = None   # parallel.Communicator for the TP group (IPC one-shot all-reduce + RCCL); None = RCCL
        self.weight_dtype = "bf16"
        self.norm_folded = False     # RMSNorm gammas folded into the consuming projections (fold_norms)
        self._ssq = None             # decode: per-(row, 16-column tile) sums of squares of the residual stream

    # ------------------------------------------------------------------ weights
    @torch.no_grad()
    def random_init(self, seed: int = 0):
        """Per-rank random shards generated on the model's device (coherent full model)."""
        dev = self.embed.device
        g = torch.Generator(device=dev).manual_seed(seed * 1000 + self.tp.rank)
        Hd = self.cfg.hidden_size
        L = self.cfg.num_layers

        def rnd(p, std):
            p.copy_((torch.randn(p.shape, generator=g, device=dev, dtype=torch.float32) * std).to(p.dtype))

        self.norm_folded = False
        rnd(self.embed, 0.02)
        if self.lm_head is not None:
            rnd(self.lm_head, 0.02)
        for l in self.layers:
            rnd(l.qkv_w, Hd ** -0.5)
            rnd(l.o_w, (Hd ** -0.5) / math.sqrt(2 * L))
            rnd(l.gu_w, Hd ** -0.5)
            rnd(l.down_w, (l.I * self.tp.world) ** -0.5 / math.sqrt(2 * L))
            if self.moe:
                # unit-scale router logits for unit-RMS rows: distinct experts per token, no one-hot softmax
                rnd(l.router_w, Hd ** -0.5)
            if l.qkv_b is not None:
                rnd(l.qkv_b, 0.02)
        if self.cfg.qk_norm:
            # replicated under TP: one generator for every rank; drawn around 1 so that no test
            # passes with the gammas ignored
            gn = torch.Generator(device=dev).manual_seed(seed * 1000 + 999)
            for l in self.layers:
                for p in (l.q_norm, l.k_norm):
                    p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=gn, device=dev, dtype=torch.float32))

    @torch.no_grad()
    def load_hf_state_dict(self, sd: dict, prefix: str = "model.") -> None:
        """HF Qwen2 / Qwen3 / Llama weights (``model.layers.N.self_attn.q_proj.weight`` ...), sharded for
        this rank.  Qwen2-VL / Qwen2.5-VL / Qwen3-VL checkpoints keep the decoder under
        ``prefix="model.language_model."``.  The Qwen3 ``self_attn.{q,k}_norm.weight`` must be present exactly when
        ``cfg.qk_norm`` is set: a decoder that dropped them would serve wrong tokens silently."""
        cfg, r, w = self.cfg, self.tp.rank, self.tp.world
        D = cfg.head_dim

        def get(k):
            return sd[k].to(torch.float32)

        def rows(t, n, i):   # i-th of n equal row shards
            s = t.shape[0] // n
            return t[i * s:(i + 1) * s]

        self.norm_folded = False
        self.embed.copy_(rows(get(prefix + "embed_tokens.weight"), w, r).to(self.embed.dtype))
        if self.lm_head is not None:
            self.lm_head.copy_(rows(get("lm_head.weight"), w, r).to(self.lm_head.dtype))
        self.norm.copy_(get(prefix + "norm.weight").to(self.norm.dtype))
        kv_rep = w // cfg.num_kv_heads if w > cfg.num_kv_heads else 1
        for i, l in enumerate(self.layers):
            p = f"{prefix}layers.{i}."
            q = rows(get(p + "self_attn.q_proj.weight"), w, r)
            kvi = r // kv_rep
            kvn = max(w // kv_rep, 1)
            k = rows(get(p + "self_attn.k_proj.weight"), kvn, kvi)
            v = rows(get(p + "self_attn.v_proj.weight"), kvn, kvi)
            l.qkv_w.copy_(torch.cat([q, k, v], 0).to(l.qkv_w.dtype))
            if l.qkv_b is not None:
                bq = rows(get(p + "self_attn.q_proj.bias"), w, r)
                bk = rows(get(p + "self_attn.k_proj.bias"), kvn, kvi)
                bv = rows(get(p + "self_attn.v_proj.bias"), kvn, kvi)
                l.qkv_b.copy_(torch.cat([bq, bk, bv], 0))
            for name, dst in (("q_norm", l.q_norm), ("k_norm", l.k_norm)):
                key = f"{p}self_attn.{name}.weight"
                if dst is not None:
                    if key not in sd:
                        raise KeyError(f"{key}: missing from the state dict of a qk_norm (Qwen3) decoder")
                    dst.copy_(get(key))
                elif key in sd:
                    raise ValueError(f"{key}: the state dict has q / k norm weights but the config has "
                                     "qk_norm=False (a Qwen3 checkpoint needs model_type 'qwen3')")
            o = get(p + "self_attn.o_proj.weight")
            l.o_w.copy_(o[:, r * l.H * D:(r + 1) * l.H * D].to(l.o_w.dtype))
            l.ln1.copy_(get(p + "input_layernorm.weight").to(l.ln1.dtype))
            l.ln2.copy_(get(p + "post_attention_layernorm.weight").to(l.ln2.dtype))
            if self.moe:
                self._load_experts(sd, p, l)
                continue
            for key in (p + "mlp.gate.weight", p + "mlp.experts.0.gate_proj.weight"):
                if key in sd:
                    raise ValueError(f"{key}: the state dict holds a mixture-of-experts MLP but the config is dense "
                                     "(num_experts = 0; a Qwen3-MoE checkpoint needs model_type 'qwen3_moe')")
            if p + "mlp.gate_proj.weight" not in sd:
                raise KeyError(f"{p}mlp.gate_proj.weight: missing from the state dict of a dense decoder")
            gate = rows(get(p + "mlp.gate_proj.weight"), w, r)
            up = rows(get(p + "mlp.up_proj.weight"), w, r)
            l.gu_w.copy_(ops.glu_interleave(gate, up).to(l.gu_w.dtype))
            dn = get(p + "mlp.down_proj.weight")
            l.down_w.copy_(dn[:, r * l.I:(r + 1) * l.I].to(l.down_w.dtype))

    def _load_experts(self, sd: dict, p: str, l) -> None:
        """The sparse MLP of layer prefix ``p``: ``mlp.gate.weight`` (router) and
        ``mlp.experts.{e}.{gate,up,down}_proj.weight``, gate and up interleaved per expert."""
        if p + "mlp.gate_proj.weight" in sd:
            raise ValueError(f"{p}mlp.gate_proj.weight: the state dict holds a dense MLP but the config has "
                             f"num_experts = {l.E}")
        keys = [p + "mlp.gate.weight"] + [f"{p}mlp.experts.{e}.{n}_proj.weight" for e in range(l.E)
                                           for n in ("gate", "up", "down")]
        for key in keys:
            if key not in sd:
                raise KeyError(f"{key}: missing from the state dict of a mixture-of-experts decoder "
                               f"(num_experts = {l.E})")
        if f"{p}mlp.experts.{l.E}.gate_proj.weight" in sd:
            raise ValueError(f"{p}mlp.experts.{l.E}.gate_proj.weight: the state dict has more experts than the "
                             f"config (num_experts = {l.E})")
        l.router_w.copy_(sd[keys[0]].to(torch.float32).to(l.router_w.dtype))
        for e in range(l.E):
            gate, up, dn = (sd[f"{p}mlp.experts.{e}.{n}_proj.weight"].to(torch.float32) for n in ("gate", "up", "down"))
            l.gu_w[e].copy_(ops.glu_interleave(gate, up).to(l.gu_w.dtype))
            l.down_w[e].copy_(dn.to(l.down_w.dtype))

    @torch.no_grad()
    def fold_norms(self) -> None:
        """Fold every RMSNorm gamma into the projection that consumes it -- W' = W * gamma[k]
        for qkv (ln1), gate|up (ln2) and an untied lm_head (final norm) -- and set the gammas
        to 1.  rms_norm(x, g) . W^T = rstd(x) * (x . W'^T), so the decode GEMMs run on the raw
        residual stream and apply rstd in their epilogue (ops.linear_dec): no norm launch and
        no normalised copy of x per token.  fp8 weights are dequantised, folded and
        requantised per row, 4-bit weights per group (same group size).  Weight loads reset
        the flag."""
        if self.norm_folded or self.moe:     # a MoE decoder keeps its norm kernels (the router reads the normalised rows)
            return

        def fold(obj, wname, gamma):
            w = getattr(obj, wname)
            sc = getattr(obj, wname[:-2] + "_s" if wname.endswith("_w") else wname + "_s", None)
            g = gamma.float()[None, :]
            for r0 in range(0, w.shape[0], 8192):            # bounded fp32 temporaries
                blk = w[r0:r0 + 8192].float()
                if w.dtype == torch.uint8:                    # 4-bit codes: [N, K / 2] + group parameters
                    blk = ops.dequantize_w4(w[r0:r0 + 8192], sc[r0:r0 + 8192]) * g
                    w4, p4 = ops.quantize_w4_rows(blk, group=2 * w.shape[1] // sc.shape[1])
                    w[r0:r0 + 8192].copy_(w4)
                    sc[r0:r0 + 8192].copy_(p4)
                elif w.dtype == torch.float8_e4m3fn:
                    blk = blk * sc[r0:r0 + 8192].float()[:, None] * g
                    w8, s8 = ops.quantize_fp8_rows(blk)
                    w[r0:r0 + 8192].copy_(w8)
                    sc[r0:r0 + 8192].copy_(s8)
                else:
                    w[r0:r0 + 8192].copy_((blk * g).to(w.dtype))

        for l in self.layers:
            fold(l, "qkv_w", l.ln1)
            l.ln1.fill_(1)
            fold(l, "gu_w", l.ln2)
            l.ln2.fill_(1)
        if self.lm_head is not None:
            fold(self, "lm_head", self.norm)
            self.norm.fill_(1)
        self.norm_folded = True

    def _ssq_buf(self, dev) -> torch.Tensor:
        if self._ssq is None or self._ssq.device != dev:
            self._ssq = torch.zeros((32, self.cfg.hidden_size // 16), device=dev, dtype=torch.float32)
        return self._ssq

    def _maybe_fold(self, x: torch.Tensor) -> None:
        # never inside a graph capture: the in-place weight rewrite would be replayed every step
        # (the engine warms up eagerly before capturing, so the fold has happened by then)
        if x.is_cuda and _FUSED_DECODE_NORM and not self.norm_folded and not self.moe and \
                not torch.cuda.is_current_stream_capturing():
            self.fold_norms()
            self._ssq_buf(x.device)

    def _quantize_experts(self, l, quant) -> None:
        """gu_w / down_w of a sparse layer -> codes of the same leading shape and the ``gu_s`` /
        ``down_s`` buffers, every expert's rows quantised on the [E * N, K] view."""
        for name in ("gu", "down"):
            w = getattr(l, name + "_w")
            E, N, K = w.shape
            codes, sc = quant(w.view(E * N, K))
            setattr(l, name + "_w", nn.Parameter(codes.view(E, N, -1), requires_grad=False))
            l.register_buffer(name + "_s", sc.view(E, N, *sc.shape[1:]), persistent=False)

    @torch.no_grad()
    def quantize_fp8(self, lm_head: bool = True, experts: bool = False) -> None:
        """fp8 decoder: QKV / o / gate|up / down (and an untied lm_head) become OCP e4m3fn
        with per-output-row fp32 scales (``<name>_s`` buffers).  Decode GEMMs (<= 32 rows)
        are HBM-bound on weights and stream the fp8 weights into bf16 MFMAs (half the bytes
        per token); prefill quantises the activations per token and runs fp8 x fp8 on the
        block-scaled matrix cores (:meth:`_f8_ok`).  Accumulation and epilogues are fp32.

        A mixture-of-experts decoder is quantised only with ``experts=True`` (ignored by a dense
        one): gate|up / down of every expert become e4m3fn with ``gu_s`` [E, 2I] / ``down_s``
        [E, H], weight-only at every row count (the grouped GEMMs of csrc/moe_wq.hip; there is no
        W8A8 sparse MLP).  The router, the embedding and the q / k norms keep their dtype."""
        if self.moe and not experts:
            raise NotImplementedError("quantize_fp8: a mixture-of-experts decoder is quantised only on request, "
                                      "quantize_fp8(experts=True) (fp8 experts in the grouped GEMMs, weight-only)")
        if self.weight_dtype == "fp8":
            return
        if self.moe and (self.cfg.hidden_size % 64 or self.cfg.moe_intermediate_size % 64):
            raise ValueError("quantize_fp8: fp8 experts need hidden_size and moe_intermediate_size to be multiples of 64")
        for l in self.layers:
            for name in ("qkv", "o") if self.moe else ("qkv", "o", "gu", "down"):
                w8, sc = ops.quantize_fp8_rows(getattr(l, name + "_w"))
                setattr(l, name + "_w", nn.Parameter(w8, requires_grad=False))
                l.register_buffer(name + "_s", sc, persistent=False)
            if self.moe:
                self._quantize_experts(l, ops.quantize_fp8_rows)
        if lm_head and self.lm_head is not None:
            w8, sc = ops.quantize_fp8_rows(self.lm_head)
            self.lm_head = nn.Parameter(w8, requires_grad=False)
            self.register_buffer("lm_head_s", sc, persistent=False)
        self.weight_dtype = "fp8"

    @torch.no_grad()
    def quantize_w4(self, lm_head: bool = True, experts: bool = False) -> None:
        """4-bit decoder (weight-only): QKV / o / gate|up / down (and an untied lm_head) become
        group-quantised 4-bit codes, uint8 [N, K / 2], with float16 (scale, wmin) per group of
        128 (32 where the local K is no multiple of 128) in the ``<name>_s`` buffers
        (ops.quantize_w4_rows).  Activations stay bf16 and accumulation fp32 at every row
        count (csrc/gemm_w4.hip); the embedding stays bf16.  The RMSNorm gammas are folded
        first (on any device) and ``norm_folded`` stays set, so the codes are never
        requantised by a later fold.

        A mixture-of-experts decoder is quantised only with ``experts=True`` (ignored by a dense
        one): gate|up / down of every expert become codes [E, N, K / 2] with ``gu_s``
        [E, 2I, H / G, 2] / ``down_s`` [E, H, I / G, 2] (csrc/moe_wq.hip).  It stays unfolded
        (``norm_folded`` False); the router, the embedding and the q / k norms keep their dtype."""
        if self.moe and not experts:
            raise NotImplementedError("quantize_w4: a mixture-of-experts decoder is quantised only on request, "
                                      "quantize_w4(experts=True) (4-bit experts in the grouped GEMMs)")
        if self.weight_dtype == "w4":
            return
        assert self.weight_dtype == "bf16", "quantize_w4 starts from float weights"
        self.fold_norms()
        for l in self.layers:
            for name in ("qkv", "o") if self.moe else ("qkv", "o", "gu", "down"):
                w = getattr(l, name + "_w")
                assert w.shape[1] % 32 == 0, f"w4: local K of {name} ({w.shape[1]}) must be a multiple of 32"
                w4, p4 = ops.quantize_w4_rows(w)
                setattr(l, name + "_w", nn.Parameter(w4, requires_grad=False))
                l.register_buffer(name + "_s", p4, persistent=False)
            if self.moe:
                self._quantize_experts(l, ops.quantize_w4_rows)
        if lm_head and self.lm_head is not None:
            w4, p4 = ops.quantize_w4_rows(self.lm_head)
            self.lm_head = nn.Parameter(w4, requires_grad=False)
            self.register_buffer("lm_head_s", p4, persistent=False)
        self.weight_dtype = "w4"

    def cache_extra(self) -> dict:
        """What a weight shard (runtime/shard_cache.py) must record next to the tensors."""
        return {"weight_dtype": self.weight_dtype, "norm_folded": bool(self.norm_folded)}

    def apply_cache_extra(self, extra: dict) -> None:
        """Restore :meth:`cache_extra` after the shard's tensors were loaded (a w4 shard holds folded
        gammas: without the flag the first GPU pass would fold, and requantise, again)."""
        self.weight_dtype = extra.get("weight_dtype", self.weight_dtype)
        self.norm_folded = bool(extra.get("norm_folded", False))

    @staticmethod
    def _lin(x, l, name, bias=None, residual=None, out=None, glu=False):
        w = getattr(l, name + "_w")
        return ops.linear(x, w, bias=bias, residual=residual, out=out, glu=glu,
                          w_scale=getattr(l, name + "_s", None))

    def _f8_ok(self, T: int) -> bool:
        """W8A8 prefill: fp8 weights, enough rows, every projection K a multiple of 128.  Never for a
        mixture-of-experts decoder: its fp8 is weight-only (there is no W8A8 sparse MLP)."""
        if self.weight_dtype != "fp8" or T < _F8_MIN_ROWS or self.moe:
            return False
        l = self.layers[0]
        return all(getattr(l, n + "_w").shape[1] % 128 == 0 for n in ("qkv", "o", "gu", "down"))

    @staticmethod
    def _lin8(x8, xs, l, name, bias=None, residual=None, out=None, glu=False):
        return ops.linear_f8(x8, xs, getattr(l, name + "_w"), getattr(l, name + "_s"), bias=bias, residual=residual,
                             out=out, glu=glu)

    # ------------------------------------------------------------------ collectives
    def _all_reduce(self, t: torch.Tensor) -> torch.Tensor:
        if self.tp.enabled:
            if self.comm is not None:
                return self.comm.all_reduce(t)
            import torch.distributed as dist

            dist.all_reduce(t, group=self.tp.group)
        return t

    def _comm_stream(self, dev: torch.device):
        """The TP group's communication stream (private: graph-safe, never PyTorch's pool)."""
        cs = getattr(self, "_cstream", None)
        if cs is None or cs.device != dev:
            cs = self._cstream = ops.private_stream(dev)
        return cs

    def _all_reduce_async(self, t: torch.Tensor):
        """Start the all-reduce of ``t`` (in place) on the communication stream once the work issued
        so far on the current stream (t's producer) is done; returns the event to wait for before
        reading ``t`` (None: it completed synchronously, e.g. on the CPU)."""
        if not t.is_cuda:
            self._all_reduce(t)
            return None
        cur = torch.cuda.current_stream(t.device)
        cs = self._comm_stream(t.device)
        cs.wait_stream(cur)
        with torch.cuda.stream(cs):
            self._all_reduce(t)
        ev = torch.cuda.Event()
        ev.record(cs)
        t.record_stream(cs)
        return ev

    @staticmethod
    def _wait(ev) -> None:
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)

    # ------------------------------------------------------------------ pieces
    def embed_tokens(self, ids: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ids [T] -> [T, hidden] (vocab-parallel: masked local lookup + all-reduce)."""
        e = ops.embed(ids.reshape(1, -1), self.embed, id_offset=self.v0,
                      out=out.view(1, -1, self.cfg.hidden_size) if out is not None else None)
        e = e.view(-1, self.cfg.hidden_size)
        return self._all_reduce(e)

    def _qk_norm(self, l) -> Optional[tuple]:
        """(q_gamma, k_gamma, eps) of a layer for the RoPE kernels (None: no q / k norm)."""
        return (l.q_norm, l.k_norm, self.cfg.rms_eps) if l.q_norm is not None else None

    def _rope_kv(self, qkv, pos, l, slots, kc, vc) -> None:
        """(q / k norm +) RoPE in place on the packed QKV rows + the paged KV-cache write of one layer.
        ``pos`` [3, T] (the prefill of a multimodal-RoPE decoder): the three-axis form of the kernels."""
        lops.rope_kv(qkv, pos, self.cos_sin, l.H, l.Hkv, self.cfg.head_dim, slots, kc, vc, qk_norm=self._qk_norm(l),
                     mrope=self.cfg.mrope if pos.dim() == 2 else None)

    def _layers(self, x: torch.Tensor, pos: torch.Tensor, slots: Optional[torch.Tensor], kv, attn_fn) -> torch.Tensor:
        """x [T, hidden] residual stream (updated in place); returns x."""
        if self._f8_ok(x.shape[0]):
            return self._layers_f8(x, pos, slots, kv, attn_fn)
        cfg = self.cfg
        eps = cfg.rms_eps
        T = x.shape[0]
        h = torch.empty_like(x)
        tp = self.tp.enabled
        # decode rows with folded norms: every RMSNorm is an rstd row scale in the epilogue of the
        # skinny GEMM that consumes it, fed by the sums of squares the producing GEMM's epilogue
        # wrote (TP keeps the norm kernel: it also adds the all-reduced row-parallel partial)
        if x.is_cuda and T <= 32 and not tp and self.norm_folded:
            return self._layers_dec(x, pos, slots, kv, attn_fn)
        if tp and T >= _TP_OVERLAP_MIN_ROWS:
            return self._layers_tp_overlap(x, pos, slots, kv, attn_fn, f8=False)
        pending: Optional[torch.Tensor] = None   # TP: row-parallel partial to add before the next norm
        for i, l in enumerate(self.layers):
            if pending is None:
                ops.rms_norm(x, l.ln1, eps, out=h)
            else:
                ops.rms_norm(x, l.ln1, eps, add=self._all_reduce(pending), resid_out=x, out=h)
            qkv = self._lin(h, l, "qkv", bias=l.qkv_b)
            kc, vc = (kv.k[i], kv.v[i]) if kv is not None else (None, None)
            if not getattr(attn_fn, "fuses_rope", False):
                self._rope_kv(qkv, pos, l, slots, kc, vc)
            att = attn_fn(qkv, l, kc, vc)                            # [T, H*D]
            if tp:
                part = self._lin(att, l, "o")
                ops.rms_norm(x, l.ln2, eps, add=self._all_reduce(part), resid_out=x, out=h)
            else:
                self._lin(att, l, "o", residual=x, out=x)
                ops.rms_norm(x, l.ln2, eps, out=h)
            if self.moe:     # sparse MLP at every row count (no TP): route, grouped expert GEMMs, combine into x
                lops.moe_mlp(h, l.router_w, l.gu_w, l.down_w, cfg.num_experts_per_tok, norm_topk=cfg.norm_topk_prob,
                             residual=x, out=x, gu_s=getattr(l, "gu_s", None), down_s=getattr(l, "down_s", None))
                del qkv, att
                continue
            g = self._lin(h, l, "gu", glu=True)
            if tp:
                pending = self._lin(g, l, "down")
            else:
                self._lin(g, l, "down", residual=x, out=x)
            del qkv, att, g
        if pending is not None:
            x.add_(self._all_reduce(pending))
        return x

    def _layers_dec(self, x, pos, slots, kv, attn_fn):
        """Decode layer stack (<= 32 rows, norms folded): 4 GEMM launches per layer and no norm
        kernel -- o / down write the residual stream plus its per-tile sums of squares
        (``ssq``), qkv / gate|up scale their rows by the rstd those give (ops.linear_dec)."""
        eps = self.cfg.rms_eps
        ssq = self._ssq_buf(x.device)
        for i, l in enumerate(self.layers):
            # layer 0 reads the embeddings (no producer GEMM): rstd from x itself
            qkv = ops.linear_dec(x, l.qkv_w, getattr(l, "qkv_s", None), bias=l.qkv_b, norm_eps=eps,
                                 ssq_in=ssq if i > 0 else None)
            kc, vc = (kv.k[i], kv.v[i]) if kv is not None else (None, None)
            if not getattr(attn_fn, "fuses_rope", False):      # decode attention rotates + caches itself
                self._rope_kv(qkv, pos, l, slots, kc, vc)
            att = attn_fn(qkv, l, kc, vc)
            ops.linear_dec(att, l.o_w, getattr(l, "o_s", None), residual=x, out=x, ssq_out=ssq)
            g = ops.linear_dec(x, l.gu_w, getattr(l, "gu_s", None), glu=True, norm_eps=eps, ssq_in=ssq)
            ops.linear_dec(g, l.down_w, getattr(l, "down_s", None), residual=x, out=x, ssq_out=ssq)
            del qkv, att, g
        return x

    def _layers_f8(self, x, pos, slots, kv, attn_fn):
        """W8A8 layer stack: every projection input is quantised per token by the kernel that
        produces it (RMSNorm+quant for qkv / gate|up, a row-quant pass for o / down) and the
        GEMMs run fp8 x fp8 (csrc/gemm_f8.hip).  Same TP structure as :meth:`_layers`."""
        cfg = self.cfg
        eps, T = cfg.rms_eps, x.shape[0]
        dev = x.device
        h8 = torch.empty((T, x.shape[1]), device=dev, dtype=torch.float8_e4m3fn)
        hs = torch.empty((T,), device=dev, dtype=torch.float32)
        tp = self.tp.enabled
        if tp and T >= _TP_OVERLAP_MIN_ROWS:
            return self._layers_tp_overlap(x, pos, slots, kv, attn_fn, f8=True)
        pending: Optional[torch.Tensor] = None
        for i, l in enumerate(self.layers):
            add = self._all_reduce(pending) if pending is not None else None
            ops.rms_norm_quant_fp8(x, l.ln1, eps, add=add, resid_out=x if add is not None else None, out=h8, scale=hs)
            qkv = self._lin8(h8, hs, l, "qkv", bias=l.qkv_b)
            kc, vc = (kv.k[i], kv.v[i]) if kv is not None else (None, None)
            self._rope_kv(qkv, pos, l, slots, kc, vc)
            att = attn_fn(qkv, l, kc, vc)                            # [T, H*D] bf16
            a8, as_ = ops.quant_rows_fp8(att)
            if tp:
                part = self._lin8(a8, as_, l, "o")
                ops.rms_norm_quant_fp8(x, l.ln2, eps, add=self._all_reduce(part), resid_out=x, out=h8, scale=hs)
            else:
                self._lin8(a8, as_, l, "o", residual=x, out=x)
                ops.rms_norm_quant_fp8(x, l.ln2, eps, out=h8, scale=hs)
            g = self._lin8(h8, hs, l, "gu", glu=True)
            g8, gs = ops.quant_rows_fp8(g)
            if tp:
                pending = self._lin8(g8, gs, l, "down")
            else:
                self._lin8(g8, gs, l, "down", residual=x, out=x)
            del qkv, att, a8, g, g8
        if pending is not None:
            x.add_(self._all_reduce(pending))
        return x

    def _layers_tp_overlap(self, x, pos, slots, kv, attn_fn, f8: bool):
        """TP prefill with the row-parallel all-reduces off the critical path.  The rows run as two
        halves A / B through every projection; each half's o / down partial is all-reduced on the
        communication stream (:meth:`_all_reduce_async`) while the compute stream carries on with
        the other half:

            o(A) -> AR(o A) | o(B) -> AR(o B) | norm(A) gu(A) down(A) -> AR(down A) | norm(B) ...

        so AR(o A) hides under o(B), AR(o B) under A's MLP, AR(down A) under B's MLP and AR(down B)
        under the next layer's A norm + qkv.  RoPE and attention run over all rows at once (every
        query needs the keys of both halves).  Same arithmetic as :meth:`_layers` / :meth:`_layers_f8`
        row for row (the reductions are per row), so TP results do not depend on the split."""
        cfg = self.cfg
        D, eps, T = cfg.head_dim, cfg.rms_eps, x.shape[0]
        dev = x.device
        # split on a 64-row boundary (GEMM row tiles), the halves as equal as that allows
        t0 = max(64, min(T - 64, (T // 2 + 32) // 64 * 64))
        halves = ((0, t0), (t0, T))
        if f8:
            h8 = torch.empty((T, x.shape[1]), device=dev, dtype=torch.float8_e4m3fn)
            hs = torch.empty((T,), device=dev, dtype=torch.float32)
        else:
            h = torch.empty_like(x)
        pend = [None, None]      # per half: row-parallel partial still to be added to x
        evs = [None, None]       # per half: its all-reduce's completion event

        def norm(i_half, gamma):
            a, b = halves[i_half]
            add = pend[i_half]
            if add is not None:
                self._wait(evs[i_half])
            xs = x[a:b]
            kw = dict(add=add, resid_out=xs) if add is not None else {}
            if f8:
                ops.rms_norm_quant_fp8(xs, gamma, eps, out=h8[a:b], scale=hs[a:b], **kw)
            else:
                ops.rms_norm(xs, gamma, eps, out=h[a:b], **kw)
            pend[i_half] = None

        def lin(i_half, l, name, inp, inp_s=None, **kw):
            a, b = halves[i_half]
            if f8:
                return self._lin8(inp[a:b], inp_s[a:b], l, name, **kw)
            return self._lin(inp[a:b], l, name, **kw)

        for i, l in enumerate(self.layers):
            nq = (l.H + 2 * l.Hkv) * D
            qkv = torch.empty((T, nq), device=dev, dtype=x.dtype)
            for c, (a, b) in enumerate(halves):
                norm(c, l.ln1)
                lin(c, l, "qkv", h8 if f8 else h, hs if f8 else None, bias=l.qkv_b, out=qkv[a:b])
            kc, vc = (kv.k[i], kv.v[i]) if kv is not None else (None, None)
            if not getattr(attn_fn, "fuses_rope", False):
                self._rope_kv(qkv, pos, l, slots, kc, vc)
            att = attn_fn(qkv, l, kc, vc)                            # [T, H*D]
            if f8:
                a8, as_ = ops.quant_rows_fp8(att)
            for c in range(2):
                pend[c] = lin(c, l, "o", a8 if f8 else att, as_ if f8 else None)
                evs[c] = self._all_reduce_async(pend[c])
            for c in range(2):
                norm(c, l.ln2)
                a, b = halves[c]
                g = lin(c, l, "gu", h8 if f8 else h, hs if f8 else None, glu=True)
                if f8:
                    g8, gs = ops.quant_rows_fp8(g)
                    pend[c] = self._lin8(g8, gs, l, "down")
                else:
                    pend[c] = self._lin(g, l, "down")
                evs[c] = self._all_reduce_async(pend[c])
            del qkv, att
        for c, (a, b) in enumerate(halves):
            self._wait(evs[c])
            x[a:b].add_(pend[c])
        return x

    def logits(self, x_rows: torch.Tensor, ssq: Optional[torch.Tensor] = None) -> torch.Tensor:
        """final norm + lm_head of rows [B, hidden] -> local-vocab fp32 logits [B, V/tp].
        With folded norms (untied head, <= 32 rows) the norm is the lm_head GEMM's rstd row
        scale; ``ssq``: the last down projection's sums of squares of these rows (decode)."""
        w = self.lm_head if self.lm_head is not None else self.embed
        ws = getattr(self, "lm_head_s", None)
        if self.norm_folded and self.lm_head is not None and x_rows.is_cuda and x_rows.shape[0] <= 32:
            return ops.linear_dec(x_rows, w, ws, norm_eps=self.cfg.rms_eps, ssq_in=ssq, out_dtype=torch.float32)
        h = ops.rms_norm(x_rows, self.norm, self.cfg.rms_eps)
        return ops.linear(h, w, out_dtype=torch.float32, w_scale=ws)

    # ------------------------------------------------------------------ forward passes
    @torch.no_grad()
    def prefill(self, x: torch.Tensor, kv=None, slots: Optional[torch.Tensor] = None, start_pos: int = 0,
                prefix_blocks: Optional[torch.Tensor] = None, pos3: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One sequence: input embeddings x [T, hidden] (modified in place) at positions
        start_pos.., k/v written to ``slots``; returns last-token logits [1, V/tp] fp32.

        ``pos3`` (a multimodal-RoPE decoder, ``cfg.mrope``): int32 [3, T] RoPE positions of *these*
        rows (``lops.mrope_positions``; default: start_pos.. on all three axes).  ``start_pos`` stays
        the rows' cache index, which the causal masks use.

        Chunked prefill (``start_pos`` > 0): ``prefix_blocks`` (int64, the sequence's KV
        blocks covering [0, start_pos + T)) — the chunk's queries attend the cached prefix
        plus themselves (causal, last query aligned with the last key).  On the GPU the paged-prefill
        kernel reads K/V of the prefix straight from the pools (``lops.paged_prefill``); the gather
        path (LUMEN_PAGED_PREFILL=0, CPU, other head dims, chunks of more than 512 rows) copies them out of the paged cache
        (K [blk, Hkv, 64, D]; V stored transposed) for the flash kernel."""
        self._maybe_fold(x)
        T = x.shape[0]
        pos = torch.arange(start_pos, start_pos + T, device=x.device, dtype=torch.int32)
        if pos3 is not None:
            if self.cfg.mrope is None:
                raise ValueError("prefill: pos3 given to a decoder without multimodal RoPE (no mrope_section)")
            if self.tp.enabled:
                raise NotImplementedError("prefill: pos3 (multimodal RoPE) is not implemented under tensor "
                                          "parallelism: the TP step messages carry no positions")
            if tuple(pos3.shape) != (3, T):
                raise ValueError(f"prefill: pos3 [3, {T}] expected, got {list(pos3.shape)}")
            pos = pos3.to(device=x.device, dtype=torch.int32).contiguous()
        elif self.cfg.mrope is not None:
            pos = pos.expand(3, T).contiguous()
        D = self.cfg.head_dim
        S = start_pos + T
        paged = start_pos > 0 and x.is_cuda and D in lops.PAGED_PREFILL_HEAD_DIMS and \
            T <= _PAGED_PREFILL_MAX_ROWS and os.environ.get("LUMEN_PAGED_PREFILL", "1") != "0"

        def attn(qkv, l, kc, vc):
            if paged and l.H // l.Hkv <= 16:
                assert prefix_blocks is not None and kc is not None, "chunked prefill needs the KV cache"
                return lops.paged_prefill(qkv, kc, vc, prefix_blocks, start_pos, l.H, l.Hkv)
            q5 = qkv.view(1, T, l.H + 2 * l.Hkv, D)
            if start_pos > 0:
                assert prefix_blocks is not None and kc is not None, "chunked prefill needs the KV cache"
                k_all, v_all = lops.gather_kv(kc, vc, prefix_blocks, S)
                k_all = k_all.to(qkv.dtype).unsqueeze(0)                      # fp8 cache -> bf16
                v_all = v_all.to(qkv.dtype).unsqueeze(0).contiguous()
            else:
                k_all, v_all = q5[:, :, l.H:l.H + l.Hkv], q5[:, :, l.H + l.Hkv:]
            o = ops.attention(q5[:, :, :l.H], k_all, v_all, causal=True)
            return o.view(T, l.H * D)

        self._layers(x, pos, slots, kv, attn)
        return self.logits(x[T - 1:T])

    @torch.no_grad()
    def decode(self, ids: torch.Tensor, pos: torch.Tensor, slots: torch.Tensor, kv, block_table: torch.Tensor,
               ctx_len: torch.Tensor, workspace: Optional[dict] = None) -> torch.Tensor:
        """B sequences, one new token each -> logits [B, V/tp] fp32."""
        x = self.embed_tokens(ids)
        self._maybe_fold(x)

        # (a q / k norm sits before the rotation, which the attention kernel's fused form does not
        # have: Qwen3 decode keeps the rope_kv launch, whose kernels apply the norm)
        fuse = _FUSED_DECODE_ROPE and x.is_cuda and self.cfg.head_dim in (64, 128) and \
            self.norm_folded and x.shape[0] <= 32 and not self.tp.enabled and kv is not None and \
            not self.cfg.qk_norm

        def attn(qkv, l, kc, vc):
            return lops.paged_decode(qkv, kc, vc, block_table, ctx_len, l.H, l.Hkv, workspace=workspace,
                                     rope=(pos, self.cos_sin, slots) if fuse else None)

        attn.fuses_rope = fuse     # read by _layers_dec: no separate rope_kv launch
        self._layers(x, pos, slots, kv, attn)
        dec = self.norm_folded and x.is_cuda and x.shape[0] <= 32 and not self.tp.enabled
        return self.logits(x, ssq=self._ssq if dec else None)

    @torch.no_grad()
    def verify(self, ids: torch.Tensor, pos: torch.Tensor, slots: torch.Tensor, kv, block_table: torch.Tensor,
               ctx_len: torch.Tensor, n_rows: torch.Tensor, T: int, workspace: Optional[dict] = None) -> torch.Tensor:
        """B sequences, up to T new tokens each (speculative decoding: the last accepted token
        and its drafts) -> logits [B*T, V/tp] fp32, row b*T + i for token i of sequence b.
        ids / pos / slots [B*T] (padding rows: slot -1); ``ctx_len`` [B] counts the cache tokens
        including this step's ``n_rows[b]`` live rows.  :meth:`decode` with
        :func:`lops.paged_verify` as the attention; RoPE and the cache write stay in rope_kv."""
        x = self.embed_tokens(ids)
        self._maybe_fold(x)

        def attn(qkv, l, kc, vc):
            return lops.paged_verify(qkv, kc, vc, block_table, ctx_len, n_rows, T, l.H, l.Hkv, workspace=workspace)

        attn.fuses_rope = False
        self._layers(x, pos, slots, kv, attn)
        dec = self.norm_folded and x.is_cuda and x.shape[0] <= 32 and not self.tp.enabled
        return self.logits(x, ssq=self._ssq if dec else None)
