"""Qwen3 decoder (per-head q / k RMSNorm before RoPE) on the CPU reference path: parity with HF
transformers (prefill + paged decode, TP=2 over gloo), loader errors, config round trips, service."""
import json
import os
import shutil
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from lumen_amd.models.llm import LLM, LLM_PRESETS, LLMConfig, TPInfo
from lumen_amd.runtime.kv_cache import PagedKVCache

transformers = pytest.importorskip("transformers")


def _cfg() -> LLMConfig:
    """2 layers, hidden 128, 4 heads x head_dim 64 (!= hidden), 2 KV heads, tied embeddings."""
    return LLMConfig(vocab_size=512, hidden_size=128, num_layers=2, num_heads=4, num_kv_heads=2, head_dim=64,
                     intermediate_size=256, rope_theta=1000000.0, rms_eps=1e-6, max_position=2048,
                     tie_word_embeddings=True, qkv_bias=False, qk_norm=True)


def _hf(cfg: LLMConfig, seed=0):
    torch.manual_seed(seed)
    hc = transformers.Qwen3Config(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size,
                                  num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.num_heads,
                                  num_key_value_heads=cfg.num_kv_heads, head_dim=cfg.head_dim,
                                  intermediate_size=cfg.intermediate_size, rope_theta=cfg.rope_theta,
                                  rms_norm_eps=cfg.rms_eps, max_position_embeddings=cfg.max_position,
                                  tie_word_embeddings=True, attention_bias=False)
    m = transformers.Qwen3ForCausalLM(hc)
    n_qk = 0
    for n, p in m.named_parameters():
        if "bias" in n:
            p.data.normal_(0, 0.1)
        if "layernorm" in n or n.endswith("norm.weight"):      # q_norm / k_norm included
            p.data.normal_(1.0, 0.1)
            n_qk += "q_norm" in n or "k_norm" in n
    assert n_qk == 2 * cfg.num_layers
    return m.eval()


def test_decoder_matches_hf():
    cfg = _cfg()
    hf = _hf(cfg)
    m = LLM(cfg, dtype=torch.float32, device="cpu")
    m.load_hf_state_dict(hf.state_dict())
    ids = torch.randint(0, cfg.vocab_size, (1, 90), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ref = hf(ids).logits[0]
    kv = PagedKVCache(cfg.num_layers, m.Hkv, cfg.head_dim, num_blocks=8, dtype=torch.float32)
    kv.blocks.reserve(5, 90)
    x = m.embed_tokens(ids[0, :70])
    lg = m.prefill(x, kv, torch.from_numpy(kv.slots(5, 0, 70)))
    assert torch.allclose(lg[0], ref[69], atol=1e-4), (lg[0] - ref[69]).abs().max()
    bt = torch.from_numpy(kv.block_table([5]))
    for p in range(70, 90):   # crosses the 64-token block boundary
        lg = m.decode(ids[0, p:p + 1], torch.tensor([p], dtype=torch.int32), torch.from_numpy(kv.slots(5, p, 1)),
                      kv, bt, torch.tensor([p + 1], dtype=torch.int32))
        assert torch.allclose(lg[0], ref[p], atol=1e-4), (p, (lg[0] - ref[p]).abs().max())


def _tp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = _cfg()
        hf = _hf(cfg)
        m = LLM(cfg, TPInfo(rank, world, None), dtype=torch.float32, device="cpu")
        m.load_hf_state_dict(hf.state_dict())
        ids = torch.randint(0, cfg.vocab_size, (1, 40), generator=torch.Generator().manual_seed(2))
        kv = PagedKVCache(cfg.num_layers, m.Hkv, cfg.head_dim, num_blocks=4, dtype=torch.float32)
        kv.blocks.reserve(1, 41)
        lg = m.prefill(m.embed_tokens(ids[0]), kv, torch.from_numpy(kv.slots(1, 0, 40)))
        parts = [torch.empty_like(lg) for _ in range(world)]
        dist.all_gather(parts, lg)
        full = torch.cat(parts, 1)
        nxt = int(full.argmax())
        lg2 = m.decode(torch.tensor([nxt]), torch.tensor([40], dtype=torch.int32),
                       torch.from_numpy(kv.slots(1, 40, 1)), kv, torch.from_numpy(kv.block_table([1])),
                       torch.tensor([41], dtype=torch.int32))
        parts2 = [torch.empty_like(lg2) for _ in range(world)]
        dist.all_gather(parts2, lg2)
        if rank == 0:
            with torch.no_grad():
                ref = hf(torch.cat([ids, torch.tensor([[nxt]])], 1)).logits[0]
            e1 = (full[0] - ref[39]).abs().max().item()
            e2 = (torch.cat(parts2, 1)[0] - ref[40]).abs().max().item()
            q.put((e1, e2))
        dist.barrier()      # tear down together: rank 1 does not close its pairs while rank 0 still computes
    finally:
        dist.destroy_process_group()


def test_tensor_parallel_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:                 # a free port: a fixed one collides with earlier runs
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    assert all(p.exitcode == 0 for p in procs)
    e1, e2 = q.get(timeout=5)
    assert e1 < 1e-4 and e2 < 1e-4, (e1, e2)


def test_loader_rejects_missing_and_unexpected_norms():
    cfg = _cfg()
    sd = _hf(cfg).state_dict()
    m = LLM(cfg, dtype=torch.float32, device="cpu")
    for name in ("q_norm", "k_norm"):
        key = f"model.layers.1.self_attn.{name}.weight"
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            m.load_hf_state_dict({k: v for k, v in sd.items() if k != key})
    # the silent failure: a Qwen3 checkpoint under a config without the norms
    plain = LLM(LLMConfig(**{**cfg.to_dict(), "qk_norm": False}), dtype=torch.float32, device="cpu")
    with pytest.raises(ValueError, match=r"model\.layers\.0\.self_attn\.q_norm\.weight"):
        plain.load_hf_state_dict(sd)
    m.load_hf_state_dict(sd)
    assert torch.equal(m.layers[1].k_norm, sd["model.layers.1.self_attn.k_norm.weight"])
    assert m.layers[0].q_norm.dtype == torch.float32 and m.layers[0].q_norm.shape == (cfg.head_dim,)


def test_config_round_trips():
    from lumen_amd.models.vlm import VLM_PRESETS, VLMConfig

    hf = {"model_type": "qwen3", "vocab_size": 151936, "hidden_size": 1024, "num_hidden_layers": 28,
          "num_attention_heads": 16, "num_key_value_heads": 8, "head_dim": 128, "intermediate_size": 3072,
          "rope_theta": 1000000, "rms_norm_eps": 1e-6, "max_position_embeddings": 40960,
          "tie_word_embeddings": True, "attention_bias": False, "bos_token_id": 151643, "eos_token_id": 151645}
    c = LLMConfig.from_hf(hf)
    assert c.qk_norm is True and c.qkv_bias is False
    assert c.head_dim == 128 and c.num_heads * c.head_dim != c.hidden_size
    assert LLMConfig.from_hf({**hf, "model_type": "qwen2"}).qk_norm is False
    assert LLMConfig.from_dict(c.to_dict()) == c
    assert LLMConfig.from_dict(json.loads(json.dumps(c.to_dict()))) == c
    assert LLMConfig.from_dict({k: v for k, v in c.to_dict().items() if k != "qk_norm"}).qk_norm is False
    v = VLM_PRESETS["tiny-qwen3"]
    assert v.llm == LLM_PRESETS["tiny-qwen3"] and v.llm.qk_norm and not v.llm.qkv_bias and v.llm.head_dim == 64
    back = VLMConfig.from_dict(json.loads(json.dumps(v.to_dict())))
    assert back.llm == v.llm and back.llm.qk_norm is True
    for name in ("qwen3-0.6b", "qwen3-8b"):
        p = LLM_PRESETS[name]
        assert p.qk_norm and not p.qkv_bias and p.head_dim == 128


def test_state_carries_the_norms():
    """state_dict, random_init, fp8 / 4-bit quantisation and the shard-cache tensor list keep the two vectors."""
    from lumen_amd.runtime import shard_cache

    cfg = LLM_PRESETS["tiny-qwen3"]
    m = LLM(cfg, dtype=torch.float32, device="cpu")
    assert torch.equal(m.layers[0].q_norm, torch.ones(cfg.head_dim))
    m.random_init(4)
    qn, kn = m.layers[1].q_norm.clone(), m.layers[1].k_norm.clone()
    assert not torch.equal(qn, kn) and (qn - 1).abs().max() > 0.05 and (qn - 1).abs().max() < 0.6
    assert torch.equal(m.state_dict()["layers.1.q_norm"], qn)
    assert torch.equal(shard_cache._model_tensors(m)["layers.1.k_norm"], kn)
    m.quantize_w4()
    assert torch.equal(m.layers[1].q_norm, qn) and torch.equal(m.layers[1].k_norm, kn)
    m8 = LLM(cfg, dtype=torch.float32, device="cpu")
    m8.random_init(4)
    m8.quantize_fp8()
    assert torch.equal(m8.layers[1].q_norm, qn) and m8.layers[1].q_norm.dtype == torch.float32


def _serve(root, port):
    from lumen_amd.resources.validator import config_from_dict
    from lumen_amd.services.vlm import GeneralFastVLMService
    from lumen_amd.utils.image import encode_jpeg

    cfg = {"metadata": {"version": "1.0.0", "region": "other", "cache_dir": str(root)},
           "deployment": {"mode": "single", "service": "vlm"}, "server": {"port": port, "host": "127.0.0.1"},
           "services": {"vlm": {"enabled": True, "package": "lumen_vlm",
                                "import_info": {"registry_class": "lumen_vlm.fastvlm.GeneralFastVLMService",
                                                "add_to_server": "lumen_vlm.proto.ml_service_pb2_grpc.add_InferenceServicer_to_server"},
                                "backend_settings": {"device": "cpu"},
                                "models": {"general": {"model": "fastvlm-tiny-qwen3", "runtime": "onnx"}}}}}
    s = GeneralFastVLMService.from_config(config_from_dict(cfg).services["vlm"], root)
    s.initialize()
    try:
        llm = s.backend.model.llm
        assert llm.cfg.qk_norm and llm.layers[0].q_norm is not None
        img = encode_jpeg(np.random.default_rng(0).integers(0, 255, (40, 60, 3), dtype=np.uint8))
        texts = []
        for _ in range(2):
            # 32 tokens: most ids of the byte-level tokenizer decode to nothing printable, and a random
            # decoder's first few greedy tokens hardly depend on gammas drawn within 10 % of 1
            body, _, _ = s.handle("vlm_generate", img, "image/jpeg", {"prompt": "Describe.", "max_new_tokens": "32"})
            d = json.loads(body)
            assert d["generated_tokens"] == 32
            texts.append(d["text"])
        return texts, [l.q_norm.clone() for l in llm.layers]
    finally:
        s.close()


def test_service_serves_tiny_qwen3_with_the_norms(tmp_path):
    from safetensors.torch import load_file, save_file

    from lumen_amd.models.vlm import write_vlm_model

    a, b = tmp_path / "a", tmp_path / "b"
    write_vlm_model(a / "models" / "fastvlm-tiny-qwen3", "fastvlm-tiny-qwen3", preset="tiny-qwen3")
    sd = load_file(str(a / "models" / "fastvlm-tiny-qwen3" / "model.safetensors"))
    keys = [k for k in sd if k.endswith("q_norm.weight") or k.endswith("k_norm.weight")]
    assert len(keys) == 4 and all(sd[k].dtype == torch.float32 and (sd[k] - 1).abs().max() > 0.05 for k in keys)
    texts, gammas = _serve(a, 50571)
    assert texts[0] == texts[1]                                   # greedy: the same request twice
    assert torch.equal(gammas[0], sd["model.layers.0.self_attn.q_norm.weight"])
    # the same weights with both gammas set to ones
    shutil.copytree(a / "models", b / "models", ignore=shutil.ignore_patterns(".lumen_shards"))
    save_file({k: torch.ones_like(v) if k in keys else v for k, v in sd.items()},
              str(b / "models" / "fastvlm-tiny-qwen3" / "model.safetensors"))
    ones, g1 = _serve(b, 50572)
    assert torch.equal(g1[0], torch.ones_like(g1[0]))
    assert ones[0] == ones[1] and ones[0] != texts[0]
