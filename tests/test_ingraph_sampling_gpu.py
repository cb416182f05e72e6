"""Sampled and penalised requests through the decode graphs' device sampler (look-ahead included)
give, token for token, what the synchronous host sampling path gives."""
import numpy as np
import pytest
import torch

from lumen_amd.models.llm import LLM, LLM_PRESETS
from lumen_amd.runtime.engine import LLMEngine, SamplingParams
from lumen_amd.runtime.kv_cache import PagedKVCache

pytestmark = pytest.mark.gpu
CFG = LLM_PRESETS["qwen2-0.5b"]
PROMPTS = [list(np.random.default_rng(i).integers(0, 150000, 40 + 9 * i)) for i in range(4)]


@pytest.fixture(scope="module")
def model():
    m = LLM(CFG, device="cuda")
    m.random_init(5)
    return m


def _engine(m, ingraph, max_batch=4):
    kv = PagedKVCache(CFG.num_layers, m.Hkv, CFG.head_dim, num_blocks=64, device="cuda")
    return LLMEngine(m, kv, lambda ids: m.embed_tokens(torch.tensor(ids, device="cuda")), max_batch=max_batch,
                     ingraph_sampling=ingraph)


def _gen(eng, jobs):
    rs = [eng.submit(p, len(p), SamplingParams(**kw)) for p, kw in jobs]
    for r in rs:
        list(r.stream(timeout=120))
    return [list(r.tokens) for r in rs]


PENALISED = [(PROMPTS[i], dict(max_new_tokens=n, repetition_penalty=1.3)) for i, n in enumerate((6, 11, 16))]
MIXED = [(PROMPTS[0], dict(max_new_tokens=8)),
         (PROMPTS[1], dict(max_new_tokens=12, temperature=0.8, top_p=0.9, seed=1)),
         (PROMPTS[2], dict(max_new_tokens=16, temperature=1.0, top_p=1.0, repetition_penalty=1.2, seed=2))]


@pytest.fixture(scope="module")
def runs(model):
    """the same jobs on the host-sampling engine, then on the in-graph one (one model, computed once)"""
    out = {}
    for ingraph in (False, True):
        eng = _engine(model, ingraph)
        try:
            res = {"penalised": _gen(eng, PENALISED)}
            res["after_penalised"] = dict(eng.stats)
            res["mixed"] = _gen(eng, MIXED)
            res["solo_greedy"] = _gen(eng, MIXED[:1])[0]
            res["again"] = _gen(eng, MIXED[1:2])[0]
            res["stats"] = dict(eng.stats)
            res["free_slots"] = len(eng.graphs._free_slots)
        finally:
            eng.close()
        out[ingraph] = res
    return out


def test_penalised_greedy_equals_the_host_path(runs):
    # different lengths: requests leave the batch at different steps, so look-ahead steps are discarded
    assert runs[True]["penalised"] == runs[False]["penalised"]
    assert [len(t) for t in runs[True]["penalised"]] == [6, 11, 16]
    st = runs[True]["after_penalised"]
    assert st.get("ingraph_sample_steps", 0) > 0 and st.get("lookahead_steps", 0) > 0
    assert not runs[False]["stats"].get("ingraph_sample_steps", 0)


def test_mixed_batch_equals_the_host_path(runs):
    assert runs[True]["mixed"] == runs[False]["mixed"]
    assert [len(t) for t in runs[True]["mixed"]] == [8, 12, 16]
    # the greedy request next to sampled ones: its solo greedy run, up to bf16 batch-versus-solo
    # rounding (the first-two-tokens allowance of test_engine_gpu_batched)
    assert runs[True]["mixed"][0][:2] == runs[True]["solo_greedy"][:2]
    assert runs[True]["again"] == runs[False]["again"]          # the sampled request alone
    assert runs[True]["free_slots"] == 4, "a finished request kept its bitmap slot"


def test_seed_determinism_and_slot_reuse(model):
    """max_batch = 2 and two waves of two penalised requests: the second wave reuses the bitmap slots of
    the first and must still equal the host engine (a slot that was not cleared would penalise the
    first wave's tokens)"""
    wave = lambda a, b: [(PROMPTS[a], dict(max_new_tokens=9, repetition_penalty=1.3, temperature=0.9, seed=3)),  # noqa: E731
                         (PROMPTS[b], dict(max_new_tokens=12, repetition_penalty=1.2))]
    out = {}
    for ingraph in (False, True):
        eng = _engine(model, ingraph, max_batch=2)
        try:
            out[ingraph] = [_gen(eng, wave(0, 1)), _gen(eng, wave(2, 3)), _gen(eng, wave(2, 3))]
            if ingraph:
                assert eng.stats.get("ingraph_sample_steps", 0) > 0
                assert eng.graphs.seen.shape[0] == 2 and len(eng.graphs._free_slots) == 2
        finally:
            eng.close()
    assert out[True][1] == out[False][1], "second wave differs from the host path"
    assert out[True][0] == out[False][0]
    assert out[True][2] == out[True][1], "the same seed twice gave different tokens"


def test_env_switch_turns_it_off(model, monkeypatch):
    monkeypatch.setenv("LUMEN_INGRAPH_SAMPLING", "0")
    eng = _engine(model, None)
    try:
        assert eng.ingraph_sampling is False
        toks = _gen(eng, PENALISED[:1])
        assert len(toks[0]) == 6
        assert not eng.stats.get("ingraph_sample_steps", 0)
    finally:
        eng.close()
