"""Multimodal RoPE (Qwen2-VL / Qwen2.5-VL / Qwen3-VL decoders) on the CPU reference path: the axis
maps, the rope_kv reference against HF's formulation, image position ids, config parsing, chunked
prefill through a paged cache, and the engine (chunks, prefix cache, speculative decoding) against
a hand-driven prefill(pos3) + decode(ctx + delta) loop."""
import hashlib

import numpy as np
import pytest
import torch

from lumen_amd.models.llm import LLM, LLM_PRESETS, LLMConfig, TPInfo
from lumen_amd.models.vlm import VLM, VLM_PRESETS
from lumen_amd.ops import llm as lops
from lumen_amd.runtime.engine import LLMEngine, SamplingParams
from lumen_amd.runtime.kv_cache import PagedKVCache
from lumen_amd.services.vlm.backend import prefix_cache_keys

IMG = 259                    # image_token_id of the tiny presets
TOL = 1e-4                   # tests/test_qwen3_cpu.py's fp32 logit tolerance


# ------------------------------------------------------------------ axis maps
def test_axes_contiguous_literal():
    ax = lops.mrope_axes(128, [16, 24, 24])
    assert ax.dtype == torch.uint8 and ax.tolist() == [0] * 16 + [1] * 24 + [2] * 24


def test_axes_interleaved_literal():
    ax = lops.mrope_axes(128, [24, 20, 20], True).tolist()
    assert [i for i, a in enumerate(ax) if a == 1] == list(range(1, 59, 3))          # 1, 4, ..., 58
    assert [i for i, a in enumerate(ax) if a == 2] == list(range(2, 60, 3))          # 2, 5, ..., 59
    assert [i for i, a in enumerate(ax) if a == 0] == list(range(0, 60, 3)) + [60, 61, 62, 63]
    assert ax.count(0) == 24 and ax.count(1) == 20 and ax.count(2) == 20


def test_axes_refuse_bad_sections():
    with pytest.raises(ValueError, match="sum to head_dim / 2"):
        lops.mrope_axes(128, [16, 24, 23])
    with pytest.raises(ValueError, match="three sections"):
        lops.mrope_axes(128, [32, 32])
    # the returned map is the caller's own: writing to it does not change the next one
    a = lops.mrope_axes(64, [8, 12, 12])
    a.fill_(2)
    assert lops.mrope_axes(64, [8, 12, 12]).tolist() == [0] * 8 + [1] * 12 + [2] * 12


# ------------------------------------------------------------------ rope_kv reference vs HF's formulation
def _hf_mrope(x, pos3, cos_sin, sections, interleaved):
    """HF apply_multimodal_rotary_pos_emb / apply_interleaved_mrope on x [T, n, D] fp32: D-wide cos and
    sin per axis ([3, T, D], the half-width angles repeated twice), then chunks of the doubled sections
    taken from axis i % 3 (contiguous) or strided slices of the h and w rows written over the t row
    (interleaved), then x * cos + rotate_half(x) * sin."""
    cs = cos_sin[pos3.long()]                                          # [3, T, D/2, 2]
    if interleaved:
        c, s = cs[0, ..., 0].clone(), cs[0, ..., 1].clone()            # [T, D/2]: start from the t row
        for dim, off in ((1, 1), (2, 2)):
            sl = slice(off, sections[dim] * 3, 3)
            c[:, sl], s[:, sl] = cs[dim, :, sl, 0], cs[dim, :, sl, 1]
        cos, sin = torch.cat([c, c], -1), torch.cat([s, s], -1)
    else:
        cos3 = torch.cat([cs[..., 0], cs[..., 0]], -1)                 # [3, T, D]
        sin3 = torch.cat([cs[..., 1], cs[..., 1]], -1)
        cos = torch.cat([m[i % 3] for i, m in enumerate(cos3.split(list(sections) * 2, dim=-1))], -1)
        sin = torch.cat([m[i % 3] for i, m in enumerate(sin3.split(list(sections) * 2, dim=-1))], -1)
    half = x.shape[-1] // 2
    rot = torch.cat([-x[..., half:], x[..., :half]], -1)
    return x * cos[:, None, :] + rot * sin[:, None, :]


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("D,sections,interleaved", [(128, (16, 24, 24), False), (128, (24, 20, 20), True),
                                                    (64, (8, 12, 12), False), (64, (12, 10, 10), True)])
def test_rope_kv_reference_matches_hf_formulation(D, sections, interleaved, norm):
    T, H, Hkv = 9, 3, 2
    g = torch.Generator().manual_seed(D + interleaved + 2 * norm)
    qkv = torch.randn(T, (H + 2 * Hkv) * D, generator=g)
    pos3 = torch.randint(0, 4000, (3, T), generator=g, dtype=torch.int32)
    assert not torch.equal(pos3[0], pos3[1]) and not torch.equal(pos3[1], pos3[2]) and not torch.equal(pos3[0], pos3[2])
    cs = lops.rope_cos_sin(4096, D, 1e6)
    qk = (torch.rand(D, generator=g) + 0.5, torch.rand(D, generator=g) + 0.5, 1e-6) if norm else None
    got = qkv.clone()
    lops.rope_kv(got, pos3, cs, H, Hkv, D, qk_norm=qk, mrope=(sections, interleaved))
    x = qkv[:, :(H + Hkv) * D].view(T, H + Hkv, D)
    if norm:
        x = lops._qk_norm_ref(x, H, qk)
    want = _hf_mrope(x, pos3, cs, sections, interleaved).reshape(T, -1)
    assert torch.allclose(got[:, :(H + Hkv) * D], want, atol=1e-6, rtol=0)
    assert torch.equal(got[:, (H + Hkv) * D:], qkv[:, (H + Hkv) * D:])
    # equal axes: the three-axis form is the 1-D form, exactly
    one = qkv.clone()
    lops.rope_kv(one, pos3[1], cs, H, Hkv, D, qk_norm=qk)
    same = qkv.clone()
    lops.rope_kv(same, pos3[1].expand(3, T), cs, H, Hkv, D, qk_norm=qk, mrope=(sections, interleaved))
    assert torch.equal(one, same)


def test_rope_kv_argument_errors():
    D, T = 64, 4
    qkv = torch.zeros(T, 4 * D)
    cs = lops.rope_cos_sin(64, D)
    p1, p3 = torch.zeros(T, dtype=torch.int32), torch.zeros(3, T, dtype=torch.int32)
    with pytest.raises(ValueError, match="sum to head_dim / 2"):
        lops.rope_kv(qkv, p3, cs, 2, 1, D, mrope=((8, 12, 13), False))
    with pytest.raises(ValueError, match="three sections"):
        lops.rope_kv(qkv, p3, cs, 2, 1, D, mrope=((16, 16), False))
    with pytest.raises(ValueError, match=r"pos \[3, 4\]"):
        lops.rope_kv(qkv, p1, cs, 2, 1, D, mrope=((8, 12, 12), False))
    with pytest.raises(ValueError, match="needs mrope"):
        lops.rope_kv(qkv, p3, cs, 2, 1, D)


# ------------------------------------------------------------------ positions
def test_positions_two_images_literal():
    ids = [5, 6] + [IMG] * 16 + [7] + [IMG] * 16 + [8, 9]
    pos, delta = lops.mrope_positions(ids, IMG, (4, 4))
    assert pos.dtype == torch.int32 and tuple(pos.shape) == (3, 37) and delta == -24
    t = [0, 1] + [2] * 16 + [6] + [7] * 16 + [11, 12]
    h = [0, 1] + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [6] + [7] * 4 + [8] * 4 + [9] * 4 + [10] * 4 + [11, 12]
    w = [0, 1] + [2, 3, 4, 5] * 4 + [6] + [7, 8, 9, 10] * 4 + [11, 12]
    assert pos.tolist() == [t, h, w]
    assert int(pos.max()) + 1 - len(ids) == delta


def test_positions_without_image_and_rectangular_grid():
    pos, delta = lops.mrope_positions([3, 4, 5, 6], IMG, (4, 4))
    assert delta == 0 and pos.tolist() == [[0, 1, 2, 3]] * 3
    # a 2 x 3 grid advances by max(2, 3); a short run of placeholders is text
    pos, delta = lops.mrope_positions([1] + [IMG] * 6 + [2, IMG], IMG, (2, 3))
    assert pos.tolist() == [[0, 1, 1, 1, 1, 1, 1, 4, 5], [0, 1, 1, 1, 2, 2, 2, 4, 5], [0, 1, 2, 3, 1, 2, 3, 4, 5]]
    assert delta == -3


def test_vlm_rope_positions():
    m = VLM(VLM_PRESETS["tiny-qwen3vl"], dtype=torch.float32, device="cpu")
    full, starts = m.expand_image_tokens([4, IMG, 5], 1)
    pos, delta = m.rope_positions(full)
    assert starts == [1] and len(full) == 18 and delta == -12
    want, _ = lops.mrope_positions(full, IMG, (4, 4))
    assert torch.equal(pos, want)
    assert VLM(VLM_PRESETS["tiny-qwen3"], dtype=torch.float32, device="cpu").rope_positions(full) is None
    assert VLM_PRESETS["tiny-qwen2vl"].llm.mrope == ((8, 12, 12), False)


# ------------------------------------------------------------------ configs
_HF_TEXT = dict(vocab_size=512, hidden_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                intermediate_size=256, rope_theta=1e6, rms_norm_eps=1e-6, max_position_embeddings=2048)
_RS2 = {"type": "mrope", "mrope_section": [4, 6, 6]}
_RS3 = {"rope_type": "default", "mrope_section": [12, 10, 10], "mrope_interleaved": True}


@pytest.mark.parametrize("mt", ["qwen2_vl", "qwen2_5_vl", "qwen2_vl_text", "qwen2_5_vl_text"])
def test_from_hf_qwen2_vl_types(mt):
    flat = LLMConfig.from_hf({**_HF_TEXT, "model_type": mt, "rope_scaling": _RS2})
    assert flat.mrope == ((4, 6, 6), False) and flat.qkv_bias and not flat.qk_norm and flat.head_dim == 32
    assert flat.rope_scaling == _RS2
    if not mt.endswith("_text"):      # the VLM config with the decoder under text_config
        nested = LLMConfig.from_hf({"model_type": mt, "vision_config": {"depth": 2},
                                    "text_config": {**_HF_TEXT, "model_type": mt + "_text", "rope_scaling": _RS2}})
        assert nested == flat


@pytest.mark.parametrize("mt", ["qwen3_vl", "qwen3_vl_text"])
def test_from_hf_qwen3_vl_types(mt):
    text = {**_HF_TEXT, "head_dim": 64, "model_type": "qwen3_vl_text", "rope_scaling": _RS3}
    c = LLMConfig.from_hf(text if mt.endswith("_text") else {"model_type": mt, "text_config": text})
    assert c.mrope == ((12, 10, 10), True) and c.qk_norm and not c.qkv_bias and c.head_dim == 64
    assert c.rope_theta == 1e6 and c.max_position == 2048
    # newer HF configs: the same dict under rope_parameters, rope_theta inside it
    t2 = {k: v for k, v in text.items() if k not in ("rope_scaling", "rope_theta")}
    c2 = LLMConfig.from_hf({**t2, "rope_parameters": {**_RS3, "rope_theta": 1e6}})
    assert c2.mrope == c.mrope and c2.rope_theta == 1e6


def test_from_hf_refusals_and_plain_types():
    for cfg in ({**_HF_TEXT, "model_type": "qwen3_vl_moe_text"},
                {"model_type": "qwen3_vl_moe", "text_config": {**_HF_TEXT, "model_type": "qwen3_vl_moe_text"}}):
        with pytest.raises(ValueError, match="qwen3_vl_moe"):
            LLMConfig.from_hf(cfg)
    bad = LLMConfig.from_hf({**_HF_TEXT, "model_type": "qwen2_vl", "rope_scaling": {"mrope_section": [4, 6, 7]}})
    with pytest.raises(ValueError, match="sum to head_dim / 2"):
        bad.mrope
    assert LLMConfig.from_hf({**_HF_TEXT, "model_type": "qwen2"}).mrope is None
    assert LLMConfig.from_hf({**_HF_TEXT, "model_type": "llama",
                              "rope_scaling": {"rope_type": "llama3", "factor": 8.0}}).mrope is None
    assert LLM_PRESETS["tiny-qwen2vl"].mrope == ((8, 12, 12), False) and LLM_PRESETS["tiny-qwen2vl"].qkv_bias
    assert LLM_PRESETS["tiny-qwen3vl"].mrope == ((12, 10, 10), True) and LLM_PRESETS["tiny-qwen3vl"].qk_norm
    assert LLMConfig.from_dict(LLM_PRESETS["tiny-qwen3vl"].to_dict()) == LLM_PRESETS["tiny-qwen3vl"]


@pytest.mark.parametrize("kind", ["qwen2_vl", "qwen3_vl"])
def test_decoder_matches_hf_text_model(kind):
    """The decoder with three-axis positions against HF's Qwen2-VL / Qwen3-VL text model, weights
    loaded from its state dict under the ``model.language_model.`` prefix of those checkpoints."""
    tr = pytest.importorskip("transformers")
    if kind == "qwen2_vl":
        hc = tr.Qwen2VLTextConfig(**{**_HF_TEXT, "num_attention_heads": 2, "tie_word_embeddings": True,
                                     "rope_scaling": {"type": "mrope", "mrope_section": [8, 12, 12]}})
        cls = tr.Qwen2VLTextModel
    else:
        hc = tr.Qwen3VLTextConfig(**{**_HF_TEXT, "head_dim": 64, "tie_word_embeddings": True, "rope_scaling": _RS3})
        cls = tr.Qwen3VLTextModel
    torch.manual_seed(0)
    hf = cls(hc).eval()
    for n, p in hf.named_parameters():
        if "bias" in n:
            p.data.normal_(0, 0.1)
        if "layernorm" in n or n.endswith("norm.weight"):
            p.data.normal_(1.0, 0.1)
    cfg = LLMConfig.from_hf(hc.to_dict())
    cfg.tie_word_embeddings = True
    assert cfg.mrope is not None and cfg.head_dim == 64
    m = LLM(cfg, dtype=torch.float32, device="cpu")
    m.load_hf_state_dict({"model.language_model." + k: v for k, v in hf.state_dict().items()},
                         prefix="model.language_model.")
    ids = [5, 6] + [IMG] * 16 + [7, 8, 9] + [IMG] * 16 + [10, 11]
    pos3, _ = lops.mrope_positions(ids, IMG, (4, 4))
    t = torch.tensor(ids)
    with torch.no_grad():
        hid = hf(input_ids=t[None], position_ids=pos3.long()[:, None, :]).last_hidden_state[0]
    ref = hid[-1:] @ hf.embed_tokens.weight.T
    got = m.prefill(m.embed_tokens(t), pos3=pos3)
    assert torch.allclose(got, ref, atol=TOL), (got - ref).abs().max()


# ------------------------------------------------------------------ model
def _llm(preset="tiny-qwen3vl", seed=3):
    m = LLM(LLM_PRESETS[preset], dtype=torch.float32, device="cpu")
    m.random_init(seed)
    return m


def _prompt(n_before=10, n_after=50, seed=0):
    g = np.random.default_rng(seed)
    ids = [int(t) for t in g.integers(0, IMG, n_before)] + [IMG] * 16 + [int(t) for t in g.integers(0, IMG, n_after)]
    pos3, delta = lops.mrope_positions(ids, IMG, (4, 4))
    return ids, pos3, delta


def _kv(m, blocks=8):
    return PagedKVCache(m.cfg.num_layers, m.Hkv, m.cfg.head_dim, num_blocks=blocks, dtype=torch.float32)


@pytest.mark.parametrize("preset", ["tiny-qwen2vl", "tiny-qwen3vl"])
def test_prefill_chunks_cut_inside_the_image(preset):
    m = _llm(preset)
    ids, pos3, delta = _prompt()
    assert delta == -12
    T = len(ids)
    x = m.embed_tokens(torch.tensor(ids))
    kv = _kv(m)
    kv.blocks.reserve(1, T)
    whole = m.prefill(x.clone(), kv, torch.from_numpy(kv.slots(1, 0, T)), pos3=pos3)
    kv2 = _kv(m)
    kv2.blocks.reserve(1, T)
    lg = None
    for s, e in ((0, 13), (13, 20), (20, 70), (70, T)):      # rows 10 .. 25 are the image
        tab = torch.from_numpy(np.asarray(kv2.blocks.table(1), np.int64)[: -(-e // 64)]) if s else None
        lg = m.prefill(x[s:e].clone(), kv2, torch.from_numpy(kv2.slots(1, s, e - s)), start_pos=s, prefix_blocks=tab,
                       pos3=pos3[:, s:e])
    assert torch.allclose(lg, whole, atol=TOL), (lg - whole).abs().max()
    # sensitivity: the image's positions matter far beyond the tolerance, so a forgotten delta or a
    # chunk fed arange positions cannot pass the tests below
    flat = m.prefill(x.clone(), pos3=torch.arange(T, dtype=torch.int32).expand(3, T))
    assert (flat - whole).abs().max().item() > 100 * TOL, (flat - whole).abs().max()


def test_equal_axes_equal_the_default_exactly():
    m = _llm()
    ids, _, _ = _prompt()
    T = len(ids)
    x = m.embed_tokens(torch.tensor(ids))
    assert torch.equal(m.prefill(x.clone(), pos3=torch.arange(T, dtype=torch.int32).expand(3, T)), m.prefill(x.clone()))
    # and the three-axis form on equal axes is the 1-D decoder holding the same tensors
    plain = LLM(LLM_PRESETS["tiny-qwen3"], dtype=torch.float32, device="cpu")
    plain.load_state_dict(m.state_dict())
    assert torch.equal(plain.prefill(x.clone()), m.prefill(x.clone()))


def test_prefill_refusals():
    m = _llm()
    x = torch.zeros(4, m.cfg.hidden_size)
    with pytest.raises(ValueError, match=r"pos3 \[3, 4\]"):
        m.prefill(x, pos3=torch.zeros(3, 5, dtype=torch.int32))
    plain = LLM(LLM_PRESETS["tiny-qwen3"], dtype=torch.float32, device="cpu")
    with pytest.raises(ValueError, match="without multimodal RoPE"):
        plain.prefill(x, pos3=torch.zeros(3, 4, dtype=torch.int32))
    tp = LLM(LLM_PRESETS["tiny-qwen3vl"], TPInfo(0, 2, None), dtype=torch.float32, device="cpu")
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        tp.prefill(x, pos3=torch.zeros(3, 4, dtype=torch.int32))


# ------------------------------------------------------------------ engine
NEW = 12


@pytest.fixture(scope="module")
def vlm():
    """tiny-qwen3vl end to end: the ViT tower, the projector and the multimodal-RoPE decoder"""
    m = VLM(VLM_PRESETS["tiny-qwen3vl"], dtype=torch.float32, device="cpu")
    m.random_init(5)
    return m.eval()


def _image(seed=0):
    return torch.randint(0, 256, (32, 32, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _request(vlm, seed=0, n_after=50):
    g = np.random.default_rng(seed)
    ids = [int(t) for t in g.integers(0, IMG, 10)] + [IMG] + [int(t) for t in g.integers(0, IMG, n_after)]
    full, starts = vlm.expand_image_tokens(ids, 1)
    pos3, delta = vlm.rope_positions(full)
    assert starts == [10] and delta == -12
    return ids, full, pos3, delta


def _hand_loop(vlm, ids, img, pos3, delta, n):
    """prefill with the three-axis positions, then greedy decode steps at cache index + delta"""
    m = vlm.llm
    x = vlm.build_prefill(ids, [img])
    T = x.shape[0]
    kv = _kv(m)
    kv.blocks.reserve(1, T + n)
    lg = m.prefill(x, kv, torch.from_numpy(kv.slots(1, 0, T)), pos3=pos3)
    bt = torch.from_numpy(kv.block_table([1]))
    toks = []
    for i in range(n):
        toks.append(int(lg[0].argmax()))
        lg = m.decode(torch.tensor(toks[-1:]), torch.tensor([T + i + delta], dtype=torch.int32),
                      torch.from_numpy(kv.slots(1, T + i, 1)), kv, bt, torch.tensor([T + i + 1], dtype=torch.int32))
    return toks


def _engine(vlm, **kw):
    m = vlm.llm
    return LLMEngine(m, _kv(m, 16), lambda a: vlm.build_prefill(a[0], [a[1]]), max_batch=4, **kw)


def _generate(eng, ids, full, img, pos3, keys=None, n=NEW):
    r = eng.submit((ids, img), len(full), SamplingParams(max_new_tokens=n), prompt_ids=full, rope_pos=pos3,
                   prefix_keys=keys)
    for _ in r.stream(timeout=120):
        pass
    return r


def test_engine_matches_hand_loop(vlm, monkeypatch):
    monkeypatch.delenv("LUMEN_SPEC_DECODE", raising=False)
    ids, full, pos3, delta = _request(vlm)
    img = _image()
    want = _hand_loop(vlm, ids, img, pos3, delta, NEW)
    # the delta shows in the tokens: the same loop at the cache index leaves them
    assert _hand_loop(vlm, ids, img, pos3, 0, NEW) != want
    eng = _engine(vlm)
    try:
        r = _generate(eng, ids, full, img, pos3)
        assert r.tokens == want and r.rope_delta == delta and eng.stats["prefill_chunks"] == 1
    finally:
        eng.close()
    eng = _engine(vlm, prefill_chunk=16)       # chunks [0, 16) [16, 32) ...: two cuts inside the image rows 10 .. 25
    try:
        r = _generate(eng, ids, full, img, pos3)
        assert r.tokens == want and eng.stats["prefill_chunks"] == -(-len(full) // 16)
    finally:
        eng.close()


def test_engine_prefix_hit_keeps_the_positions(vlm, monkeypatch):
    """The second request shares the first 64 tokens (the image included) and differs after them: it
    prefills only rows 64 .., whose positions are the columns 64 .. of its own rope_pos."""
    monkeypatch.delenv("LUMEN_SPEC_DECODE", raising=False)
    img = _image()
    digest = hashlib.blake2b(img.numpy().tobytes(), digest_size=16).digest()
    ids, full, pos3, delta = _request(vlm, n_after=60)
    ids2 = ids[:-6] + [int(t) for t in np.random.default_rng(9).integers(0, IMG, 6)]
    full2, _ = vlm.expand_image_tokens(ids2, 1)
    pos3b, delta2 = vlm.rope_positions(full2)
    assert full2[:64] == full[:64] and full2 != full and delta2 == delta
    eng = _engine(vlm)
    try:
        r1 = _generate(eng, ids, full, img, pos3, keys=prefix_cache_keys(full, [10], digest))
        r2 = _generate(eng, ids2, full2, img, pos3b, keys=prefix_cache_keys(full2, [10], digest))
        assert r1.cached_tokens == 0 and r2.cached_tokens == 64 and eng.stats["prefix_hits"] == 1
        assert r1.tokens == _hand_loop(vlm, ids, img, pos3, delta, NEW)
        assert r2.tokens == _hand_loop(vlm, ids2, img, pos3b, delta2, NEW)
    finally:
        eng.close()


def test_engine_speculative_decoding(vlm, monkeypatch):
    """verify steps feed ctx + delta + arange(n): a repetitive continuation makes the n-gram drafter
    propose, and the tokens stay those of the hand-driven loop"""
    monkeypatch.setenv("LUMEN_SPEC_DECODE", "ngram")
    ids, full, pos3, delta = _request(vlm)
    img = _image()
    want = _hand_loop(vlm, ids, img, pos3, delta, 32)
    eng = _engine(vlm)
    try:
        r = _generate(eng, ids, full, img, pos3, n=32)
        assert r.tokens == want
        assert eng.stats["spec_steps"] > 0, eng.stats
    finally:
        eng.close()


def test_submit_validation(vlm, monkeypatch):
    monkeypatch.delenv("LUMEN_SPEC_DECODE", raising=False)
    ids, full, pos3, _ = _request(vlm)
    T = len(full)
    sp = lambda n=4: SamplingParams(max_new_tokens=n)  # noqa: E731
    eng = _engine(vlm)
    try:
        with pytest.raises(ValueError, match=rf"\[3, {T}\]"):
            eng.submit((ids, None), T, sp(), rope_pos=pos3[:, :-1])
        with pytest.raises(ValueError, match=rf"\[3, {T}\]"):
            eng.submit((ids, None), T, sp(), rope_pos=pos3[0])
        with pytest.raises(ValueError, match=rf"\[3, {T}\]"):
            eng.submit((ids, None), T, sp(), rope_pos=pos3.float())
        neg = pos3.clone()
        neg[1, 3] = -1
        with pytest.raises(ValueError, match=">= 0"):
            eng.submit((ids, None), T, sp(), rope_pos=neg)
        far = pos3.clone()
        far[2, 12] = vlm.llm.cfg.max_position - 4        # + 1 + 4 new tokens: one past the table
        with pytest.raises(ValueError, match="max_position"):
            eng.submit((ids, None), T, sp(4), rope_pos=far)
        far[2, 12] -= 1                                   # exactly fits
        assert eng.submit((ids, _image()), T, sp(4), rope_pos=far).rope_delta == vlm.llm.cfg.max_position - 4 - T
    finally:
        eng.close()
    plain = VLM(VLM_PRESETS["tiny-qwen3"], dtype=torch.float32, device="cpu")
    eng = _engine(plain)
    try:
        with pytest.raises(ValueError, match="without multimodal RoPE"):
            eng.submit((ids, None), T, sp(), rope_pos=pos3)
    finally:
        eng.close()


# ------------------------------------------------------------------ service
def test_service_passes_the_positions_and_refuses_tp(tmp_path, monkeypatch):
    """The VLM service on a tiny-qwen3vl pack: every request's rope_pos reaches the engine (a
    prefix-cache hit that skips the image included) and a tensor-parallel start is refused."""
    import json

    from lumen_amd.models.vlm import write_vlm_model
    from lumen_amd.resources.validator import config_from_dict
    from lumen_amd.services.vlm import GeneralFastVLMService
    from lumen_amd.services.vlm.backend import BackendError, MI355XVLMBackend
    from lumen_amd.utils.image import encode_jpeg

    monkeypatch.setenv("LUMEN_PREFIX_CACHE", "1")
    monkeypatch.delenv("LUMEN_SPEC_DECODE", raising=False)
    name = "fastvlm-tiny-qwen3vl"
    write_vlm_model(tmp_path / "models" / name, name, preset="tiny-qwen3vl")
    cfg = {"metadata": {"version": "1.0.0", "region": "other", "cache_dir": str(tmp_path)},
           "deployment": {"mode": "single", "service": "vlm"}, "server": {"port": 50581, "host": "127.0.0.1"},
           "services": {"vlm": {"enabled": True, "package": "lumen_vlm",
                                "import_info": {"registry_class": "lumen_vlm.fastvlm.GeneralFastVLMService",
                                                "add_to_server": "lumen_vlm.proto.ml_service_pb2_grpc.add_InferenceServicer_to_server"},
                                "backend_settings": {"device": "cpu"},
                                "models": {"general": {"model": name, "runtime": "onnx"}}}}}
    s = GeneralFastVLMService.from_config(config_from_dict(cfg).services["vlm"], tmp_path)
    s.initialize()
    try:
        be = s.backend
        assert be.model.cfg.llm.mrope == ((12, 10, 10), True)
        seen, submit = [], be.engine.submit
        monkeypatch.setattr(be.engine, "submit", lambda *a, **kw: (seen.append((a, kw)), submit(*a, **kw))[1])
        img = encode_jpeg(np.random.default_rng(0).integers(0, 255, (40, 60, 3), dtype=np.uint8))
        prompt = "Describe this picture in a few words, then say what is unusual about it."
        texts = []
        for _ in range(2):
            body, _, _ = s.handle("vlm_generate", img, "image/jpeg", {"prompt": prompt, "max_new_tokens": "12"})
            d = json.loads(body)
            assert d["generated_tokens"] == 12
            texts.append(d["text"])
        assert texts[0] == texts[1]                                   # greedy; the second prefills after a prefix hit
        assert be.engine.stats["prefix_hits"] == 1
        for (a, kw) in seen:
            T = a[1]
            want, delta = lops.mrope_positions(kw["prompt_ids"], be.model.cfg.image_token_id, (4, 4))
            assert T == len(kw["prompt_ids"]) > 64 and delta == -12 and torch.equal(kw["rope_pos"], want)
        with pytest.raises(BackendError, match="tensor parallelism"):
            MI355XVLMBackend(be.resources, device="cpu", tp_size=2).initialize()
    finally:
        s.close()
