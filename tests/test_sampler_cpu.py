"""The device sampler's CPU reference (ops.llm.sample_rows) draws the token the host sampling path
draws -- rep_penalty_ + the 1/T multiply + row_topk(64) + sample_from_candidates -- from the same
uniform, and the engine accepts the ``ingraph_sampling`` switch."""
import numpy as np
import pytest
import torch

from lumen_amd import ops
from lumen_amd.models.llm import LLM, LLM_PRESETS
from lumen_amd.ops import llm as lops
from lumen_amd.runtime.engine import LLMEngine, SamplingParams
from lumen_amd.runtime.kv_cache import PagedKVCache


def _bitmap(tokens, V):
    row = np.zeros(lops.seen_words(V), np.uint32)
    for t in tokens:
        row[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    return torch.from_numpy(row.view(np.int32).copy())


def _case(s, V):
    g = np.random.default_rng(1000 + s)
    logits = torch.from_numpy((g.standard_normal(V) * 3).astype(np.float32))[None]
    temp = float(g.uniform(0.3, 1.5))
    top_p = [0.5, 0.9, 1.0][int(g.integers(3))]
    pen = [1.0, 1.3][int(g.integers(2))]
    hist = [int(t) for t in g.integers(0, V, int(g.integers(1, 40)))]      # tokens generated so far, last = the input
    hist += [int(logits.argmax()), 0, V - 1][:int(g.integers(0, 4))]
    return logits, temp, top_p, pen, hist


@pytest.mark.parametrize("V,seeds", [(1000, range(200)), (20481, range(20))])
def test_reference_draws_what_the_host_path_draws(V, seeds):
    for s in seeds:
        logits, temp, top_p, pen, hist = _case(s, V)
        # today's composition
        x = logits.clone()
        lops.rep_penalty_(x, [hist], [pen])
        x.mul_(torch.tensor([1.0 / temp], dtype=torch.float32)[:, None])
        v, i, lse = ops.row_topk(x, 64, with_lse=True)
        want = lops.sample_from_candidates(v[0].numpy(), i[0].numpy(), float(lse[0]), temp, top_p,
                                           np.random.default_rng(s))
        # the sampler: the bitmap holds the tokens fed before, the last one is this step's input
        seen = torch.zeros((2, lops.seen_words(V)), dtype=torch.int32)
        seen[1] = _bitmap(hist[:-1], V)
        keep = logits.clone()
        rv, ri, rlse, tok, seen2 = lops.sample_rows(logits, [1.0 / temp], [top_p], [pen],
                                                    [np.random.default_rng(s).random()], [0], [1], seen, [hist[-1]])
        assert int(tok[0]) == want, (s, V)
        assert torch.equal(logits, keep), "the logits are read only"
        assert torch.equal(rv, v) and torch.equal(ri, i) and torch.equal(rlse, lse)
        assert torch.equal(seen2[1], _bitmap(hist, V)) and not seen2[0].any()


def test_greedy_row_and_unpenalised_slot():
    V = 1000
    logits, _, _, _, hist = _case(3, V)
    seen = torch.zeros((1, lops.seen_words(V)), dtype=torch.int32)
    top = int(logits.argmax())
    # greedy, slot -1: the arg-max, nothing marked; u is not used
    *_, tok, seen = lops.sample_rows(logits, [1.0], [1.0], [1.3], [0.999], [1], [-1], seen, [top])
    assert int(tok[0]) == top and not seen.any()
    # greedy with a penalty over the arg-max as the input token: the penalised row's arg-max
    x = logits.clone()
    lops.rep_penalty_(x, [[top]], [1.3])
    out = torch.zeros(1, dtype=torch.long)
    *_, tok, seen = lops.sample_rows(logits, [1.0], [1.0], [1.3], [0.0], [1], [0], seen, [top], out_ids=out)
    assert int(tok[0]) == int(x.argmax()) == int(out[0])
    assert torch.equal(seen[0], _bitmap([top], V))


def test_choice_consumes_one_double_per_token():
    """the engine hands the device ``rng.random()`` where the host path calls ``rng.choice``: both
    must advance the request's generator alike, for every nucleus length"""
    a, b = np.random.default_rng(5), np.random.default_rng(5)
    for n in list(range(1, 65)) * 3:
        q = np.random.default_rng(n).random(n)
        q /= q.sum()
        got = int(a.choice(n, p=q))
        c = np.cumsum(q)
        assert got == min(n - 1, int(np.searchsorted(c / c[-1], b.random(), side="right")))
    assert a.random() == b.random()


def test_engine_accepts_the_switch_and_samples_alike(monkeypatch):
    """no graphs on the CPU, so both settings take the host path: the parameter is accepted and
    the tokens are equal"""
    cfg = LLM_PRESETS["tiny"]
    m = LLM(cfg, dtype=torch.float32, device="cpu")
    m.random_init(3)
    prompts = [list(np.random.default_rng(i).integers(0, cfg.vocab_size, 20 + 7 * i)) for i in range(3)]
    params = [dict(max_new_tokens=6), dict(max_new_tokens=9, temperature=0.8, top_p=0.9, seed=1),
              dict(max_new_tokens=12, temperature=1.0, repetition_penalty=1.2, seed=2)]
    outs = {}
    for flag in (False, True, None):
        if flag is None:
            monkeypatch.setenv("LUMEN_INGRAPH_SAMPLING", "0")
        kv = PagedKVCache(cfg.num_layers, m.Hkv, cfg.head_dim, num_blocks=64, dtype=torch.float32)
        eng = LLMEngine(m, kv, lambda ids: m.embed_tokens(torch.tensor(ids)), max_batch=8, ingraph_sampling=flag)
        try:
            assert eng.ingraph_sampling is bool(flag)
            rs = [eng.submit(p, len(p), SamplingParams(**kw)) for p, kw in zip(prompts, params)]
            for r in rs:
                list(r.stream(timeout=60))
            outs[flag] = [r.tokens for r in rs]
            assert not eng.stats.get("ingraph_sample_steps", 0)
            assert all(r.seen_slot is None for r in rs)
        finally:
            eng.close()
    assert outs[True] == outs[False] == outs[None]
    assert [len(t) for t in outs[True]] == [6, 9, 12]
