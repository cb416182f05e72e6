"""Prefix KV caching on the GPU engine (Qwen2-0.5B, random weights): a prompt that extends an
earlier one starts from its published blocks, computes only the rest on the paged-prefill kernel
and generates what a cold prefill generates."""
import numpy as np
import pytest
import torch

from lumen_amd.models.llm import LLM, LLM_PRESETS
from lumen_amd.runtime.engine import LLMEngine, SamplingParams
from lumen_amd.runtime.kv_cache import PagedKVCache
from lumen_amd.services.vlm.backend import prefix_cache_keys

pytestmark = pytest.mark.gpu
CFG = LLM_PRESETS["qwen2-0.5b"]


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.float().flatten(), b.float().flatten(), dim=0).item()


@pytest.fixture(scope="module")
def model():
    m = LLM(CFG, device="cuda")
    m.random_init(8)
    return m


def _pk(ids):
    return prefix_cache_keys(ids, [], b"")


def _engine(m, dtype, graphs):
    kv = PagedKVCache(CFG.num_layers, m.Hkv, CFG.head_dim, num_blocks=48, device="cuda", dtype=dtype)
    eng = LLMEngine(m, kv, lambda ids: m.embed_tokens(torch.tensor(ids, device="cuda")), max_batch=4,
                    use_graphs=graphs)
    return eng, kv


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float8_e4m3fn], ids=["bf16", "fp8"])
def test_engine_prefix_hit(model, dtype):
    m = model
    rng = np.random.default_rng(31)
    p1 = [int(t) for t in rng.integers(0, 150000, 300)]
    p2 = p1 + [int(t) for t in rng.integers(0, 150000, 40)]
    toks = {}
    for graphs in (False, True):
        eng, kv = _engine(m, dtype, graphs)
        try:
            a = eng.submit(p1, len(p1), SamplingParams(max_new_tokens=4), prefix_keys=_pk(p1))
            list(a.stream(timeout=120))
            assert a.cached_tokens == 0 and eng.stats["prefill_tokens"] == 300 and kv.blocks.cached_blocks() == 4
            before = eng.stats["prefill_tokens"]
            b = eng.submit(p2, len(p2), SamplingParams(max_new_tokens=12), prefix_keys=_pk(p2))
            list(b.stream(timeout=120))
            assert b.cached_tokens == 256
            assert eng.stats["prefill_tokens"] - before == 84
            assert eng.stats["prefix_hits"] == 1 and eng.stats["prefix_tokens"] == 256
            assert len(b.tokens) == 12
            toks[graphs] = list(b.tokens)
            if graphs:
                assert eng.graphs is not None and eng.graphs.graphs, "decode graphs were not captured"
            else:
                # first-step logits of the warm prefill (blocks matched from the index, 84 rows on the
                # paged-prefill kernel) vs a cold prefill of the same prompt; the engine is idle
                torch.cuda.synchronize()
                assert kv.blocks.match(_pk(p2)[:4], 1001) == 256      # the blocks the first prompt published
                assert kv.blocks.reserve(1001, len(p2)) and kv.blocks.reserve(1002, len(p2))
                assert kv.blocks.table(1001)[:4] != kv.blocks.table(1002)[:4]
                ids = torch.tensor(p2, device="cuda")
                tab = torch.from_numpy(np.asarray(kv.blocks.table(1001), np.int64)).cuda()
                warm = m.prefill(m.embed_tokens(ids)[256:], kv, torch.from_numpy(kv.slots(1001, 256, 84)).cuda(),
                                 start_pos=256, prefix_blocks=tab[:-(-len(p2) // 64)])
                cold = m.prefill(m.embed_tokens(ids), kv, torch.from_numpy(kv.slots(1002, 0, len(p2))).cuda())
                torch.cuda.synchronize()
                kv.blocks.release(1001)
                kv.blocks.release(1002)
                c = _cos(warm, cold)
                print(f"warm vs cold first-step logits ({dtype}): cosine {c:.6f}")
                assert torch.isfinite(warm).all() and c > 0.999
        finally:
            eng.close()
    assert toks[True] == toks[False]
