"""The sparse mixture-of-experts MLP (Qwen3-MoE) without a GPU: the fp32 reference ops against a naive
per-token loop, the config / preset / checkpoint plumbing, the refusals, and the engine on the CPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lumen_amd import ops
from lumen_amd.models.llm import LLM, LLM_PRESETS, LLMConfig, TPInfo
from lumen_amd.models.vlm import VLM, VLM_PRESETS
from lumen_amd.ops import llm as lops
from lumen_amd.runtime.engine import LLMEngine, SamplingParams
from lumen_amd.runtime.kv_cache import PagedKVCache

CFG = LLM_PRESETS["tiny-qwen3-moe"]


def _weights(T, E, H, I, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, H, generator=g)
    gate_w = torch.randn(E, H, generator=g) * H ** -0.5
    wg = torch.randn(E, I, H, generator=g) * H ** -0.5
    wu = torch.randn(E, I, H, generator=g) * H ** -0.5
    wd = torch.randn(E, H, I, generator=g) * I ** -0.5
    gu = torch.stack([ops.glu_interleave(wg[e], wu[e]) for e in range(E)])
    return x, gate_w, wg, wu, wd, gu


def _naive(x, gate_w, wg, wu, wd, k, norm_topk=True, residual=None):
    """softmax over all experts, top-k, renormalise, down(silu(gate x) * up x), weighted sum -- token by token"""
    out = torch.zeros_like(x)
    for t in range(x.shape[0]):
        p = torch.softmax(gate_w @ x[t], dim=0)
        top = torch.topk(p, k)
        wts = top.values / top.values.sum() if norm_topk else top.values
        for wj, e in zip(wts, top.indices):
            out[t] += wj * (wd[e] @ (F.silu(wg[e] @ x[t]) * (wu[e] @ x[t])))
    return out if residual is None else out + residual


@pytest.mark.parametrize("norm_topk", [True, False])
def test_reference_matches_naive_loop(norm_topk):
    T, E, k, H, I = 9, 8, 3, 64, 32
    x, gate_w, wg, wu, wd, gu = _weights(T, E, H, I, 0)
    res = torch.randn(T, H, generator=torch.Generator().manual_seed(5))
    ref = _naive(x, gate_w, wg, wu, wd, k, norm_topk, res)
    got = lops.moe_mlp(x, gate_w, gu, wd, k, norm_topk=norm_topk, residual=res)
    assert torch.allclose(got, ref, rtol=1e-4, atol=1e-5), (got - ref).abs().max()
    ids, w = lops.moe_route(x, gate_w, k, norm_topk=norm_topk)
    assert ids.dtype == torch.int32 and w.dtype == torch.float32 and ids.shape == w.shape == (T, k)
    got2 = lops.moe_experts(x, ids, w, gu, wd, residual=res)
    assert torch.equal(got, got2)
    s = w.sum(1)
    if norm_topk:
        assert torch.allclose(s, torch.ones(T), atol=1e-6)
    else:      # un-renormalised: the chosen experts' share of the softmax over all E
        p = torch.softmax(x @ gate_w.t(), dim=1)
        assert torch.allclose(w, p.gather(1, ids.long()), rtol=1e-5, atol=1e-7)
        assert (s < 0.999).all()


def test_ties_go_to_the_lower_id():
    E, H, k = 8, 32, 3
    x = torch.ones(2, H)
    gate_w = torch.zeros(E, H)
    gate_w[5] = 1.0                      # the clear winner, then a 7-way tie at 0
    ids, w = lops.moe_route(x, gate_w, k)
    assert ids.tolist() == [[5, 0, 1], [5, 0, 1]]
    gate_w[2] = gate_w[6] = 1.0          # a 3-way tie at the top
    ids, _ = lops.moe_route(x, gate_w, k)
    assert ids.tolist() == [[2, 5, 6], [2, 5, 6]]


def test_bad_ids_and_shapes():
    T, E, k, H, I = 4, 4, 2, 64, 32
    x, gate_w, wg, wu, wd, gu = _weights(T, E, H, I, 1)
    ids, w = lops.moe_route(x, gate_w, k)
    bad = ids.clone()
    bad[0, 0], bad[2, 1] = -1, E
    got = lops.moe_experts(x, bad, w, gu, wd)
    w0 = w.clone()
    w0[0, 0] = w0[2, 1] = 0.0
    assert torch.allclose(got, lops.moe_experts(x, ids, w0, gu, wd), atol=1e-6)
    with pytest.raises(ValueError):
        lops.moe_mlp(torch.zeros(2, 48), torch.zeros(E, 48), torch.zeros(E, 64, 48), torch.zeros(E, 48, 32), k)
    with pytest.raises(ValueError):
        lops.moe_mlp(torch.zeros(2, 64), torch.zeros(E, 64), torch.zeros(E, 144, 64), torch.zeros(E, 64, 72), k)
    with pytest.raises(ValueError):
        lops.moe_route(x, gate_w, E + 1)
    with pytest.raises(ValueError):
        lops.moe_mlp(x, gate_w[:3], gu, wd, k)


HF = {"model_type": "qwen3_moe", "vocab_size": 512, "hidden_size": 128, "num_hidden_layers": 2,
      "num_attention_heads": 4, "num_key_value_heads": 2, "head_dim": 64, "intermediate_size": 256,
      "moe_intermediate_size": 64, "num_experts": 8, "num_experts_per_tok": 2, "norm_topk_prob": True,
      "decoder_sparse_step": 1, "mlp_only_layers": [], "rope_theta": 1000000.0, "max_position_embeddings": 2048,
      "tie_word_embeddings": True, "bos_token_id": 1, "eos_token_id": 2}


def test_from_hf_reads_the_moe_fields():
    c = LLMConfig.from_hf(HF)
    assert (c.num_experts, c.num_experts_per_tok, c.moe_intermediate_size, c.norm_topk_prob) == (8, 2, 64, True)
    assert c.qk_norm and not c.qkv_bias
    assert LLMConfig.from_hf({**HF, "norm_topk_prob": False}).norm_topk_prob is False
    assert LLMConfig.from_dict(c.to_dict()) == c
    with pytest.raises(ValueError, match="mlp_only_layers"):
        LLMConfig.from_hf({**HF, "mlp_only_layers": [0]})
    with pytest.raises(ValueError, match="decoder_sparse_step"):
        LLMConfig.from_hf({**HF, "decoder_sparse_step": 2})
    dense = LLMConfig.from_hf({**HF, "model_type": "qwen3"})
    assert dense.num_experts == 0 and dense.qk_norm


def test_presets():
    big = LLM_PRESETS["qwen3-30b-a3b"]
    assert (big.hidden_size, big.num_layers, big.num_heads, big.num_kv_heads, big.head_dim) == (2048, 48, 32, 4, 128)
    assert (big.num_experts, big.num_experts_per_tok, big.moe_intermediate_size) == (128, 8, 768)
    assert big.vocab_size == 151936 and not big.tie_word_embeddings and big.qk_norm
    tiny, base = LLM_PRESETS["tiny-qwen3-moe"], LLM_PRESETS["tiny-qwen3"]
    assert (tiny.num_experts, tiny.num_experts_per_tok, tiny.moe_intermediate_size) == (8, 2, 64)
    assert (tiny.hidden_size, tiny.num_heads, tiny.head_dim, tiny.qk_norm) == \
        (base.hidden_size, base.num_heads, base.head_dim, True)
    assert VLM_PRESETS["tiny-qwen3-moe"].llm == tiny
    assert LLM_PRESETS["tiny-qwen3"].num_experts == 0


def _model(seed=1):
    m = LLM(CFG, dtype=torch.float32, device="cpu")
    m.random_init(seed)
    return m


def test_layer_tensors_and_forward():
    m = _model()
    l = m.layers[0]
    E, I, H = CFG.num_experts, CFG.moe_intermediate_size, CFG.hidden_size
    assert l.router_w.shape == (E, H) and l.gu_w.shape == (E, 2 * I, H) and l.down_w.shape == (E, H, I)
    assert float(l.router_w.abs().max()) > 0 and float(l.gu_w[E - 1].abs().max()) > 0
    ids = torch.randint(0, CFG.vocab_size, (12,), generator=torch.Generator().manual_seed(2))
    base = m.prefill(m.embed_tokens(ids))
    assert base.shape == (1, CFG.vocab_size) and torch.isfinite(base).all()
    m.fold_norms()
    assert not m.norm_folded, "a MoE decoder stays unfolded"
    for l in m.layers:                       # the experts matter: scramble the router and the logits move
        l.router_w.copy_(l.router_w.flip(0))
    assert (m.prefill(m.embed_tokens(ids)) - base).abs().max() > 1e-4


def test_hf_state_dict_round_trip_and_mismatches():
    v = VLM(VLM_PRESETS["tiny-qwen3-moe"], dtype=torch.float32, device="cpu")
    v.random_init(3)
    sd = v.export_state_dict()
    assert "model.layers.1.mlp.gate.weight" in sd and "model.layers.0.mlp.experts.7.down_proj.weight" in sd
    assert "model.layers.0.mlp.gate_proj.weight" not in sd
    I = CFG.moe_intermediate_size
    assert sd["model.layers.0.mlp.experts.3.up_proj.weight"].shape == (I, CFG.hidden_size)
    m = LLM(CFG, dtype=torch.float32, device="cpu")
    m.load_hf_state_dict(sd)
    for a, b in zip(m.layers, v.llm.layers):
        assert torch.equal(a.router_w, b.router_w) and torch.equal(a.gu_w, b.gu_w) and torch.equal(a.down_w, b.down_w)
        assert torch.equal(a.q_norm, b.q_norm)
    # gate / up interleaved per expert: 8 gate | 8 up rows per 16
    gu = m.layers[0].gu_w[3].view(I // 8, 2, 8, -1)
    assert torch.equal(gu[:, 0].reshape(I, -1), sd["model.layers.0.mlp.experts.3.gate_proj.weight"])
    assert torch.equal(gu[:, 1].reshape(I, -1), sd["model.layers.0.mlp.experts.3.up_proj.weight"])
    ids = torch.randint(0, CFG.vocab_size, (10,), generator=torch.Generator().manual_seed(4))
    assert torch.equal(m.prefill(m.embed_tokens(ids)), v.llm.prefill(v.llm.embed_tokens(ids)))
    # a MoE config meets a dense checkpoint
    dv = VLM(VLM_PRESETS["tiny-qwen3"], dtype=torch.float32, device="cpu")
    dv.random_init(3)
    dsd = dv.export_state_dict()
    with pytest.raises((KeyError, ValueError), match=r"mlp\.gate"):
        LLM(CFG, dtype=torch.float32, device="cpu").load_hf_state_dict(dsd)
    # ... and the reverse
    with pytest.raises((KeyError, ValueError), match=r"mlp\.(gate|experts)"):
        LLM(LLM_PRESETS["tiny-qwen3"], dtype=torch.float32, device="cpu").load_hf_state_dict(sd)
    # one expert's tensor missing: named
    part = {k: t for k, t in sd.items() if k != "model.layers.1.mlp.experts.5.up_proj.weight"}
    with pytest.raises(KeyError, match=r"layers\.1\.mlp\.experts\.5\.up_proj"):
        LLM(CFG, dtype=torch.float32, device="cpu").load_hf_state_dict(part)


def test_refusals():
    with pytest.raises(NotImplementedError, match="parallel"):
        LLM(CFG, TPInfo(rank=0, world=2), dtype=torch.float32, device="cpu")
    m = _model()
    with pytest.raises(NotImplementedError, match="quantize_fp8"):
        m.quantize_fp8()
    with pytest.raises(NotImplementedError, match="quantize_w4"):
        m.quantize_w4()
    assert m.weight_dtype == "bf16" and m.layers[0].gu_w.dtype == torch.float32


def test_engine_generates_on_cpu():
    m = _model(2)
    kv = PagedKVCache(CFG.num_layers, m.Hkv, CFG.head_dim, num_blocks=32, dtype=torch.float32)
    eng = LLMEngine(m, kv, lambda ids: m.embed_tokens(torch.tensor(ids)), max_batch=4)
    try:
        prompts = [[int(t) for t in np.random.default_rng(i).integers(0, CFG.vocab_size, 14 + 5 * i)] for i in range(3)]
        solo = []
        for p in prompts:
            r = eng.submit(p, len(p), SamplingParams(max_new_tokens=8))
            list(r.stream(timeout=60))
            solo.append(list(r.tokens))
        rs = [eng.submit(p, len(p), SamplingParams(max_new_tokens=8)) for p in prompts]
        for r, ref in zip(rs, solo):
            list(r.stream(timeout=60))
            assert list(r.tokens) == ref and len(ref) == 8
        assert eng.stats["decode_steps"] > 0
    finally:
        eng.close()
    # teacher-forced: the engine's first token is the prefill arg-max of the model itself
    lg = m.prefill(m.embed_tokens(torch.tensor(prompts[0])))
    assert int(lg.argmax()) == solo[0][0]
