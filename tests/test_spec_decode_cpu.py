"""Speculative decoding on the CPU reference path: the n-gram drafter, the paged-verify attention
reference against a naive dense causal attention, and the engine's verify step under scripted
drafters -- speculation must never change the tokens, only how many steps produce them."""
import math

import numpy as np
import pytest
import torch

from lumen_amd.models.llm import LLM, LLM_PRESETS
from lumen_amd.ops import llm as lops
from lumen_amd.runtime.engine import LLMEngine, SamplingParams
from lumen_amd.runtime.kv_cache import PagedKVCache
from lumen_amd.runtime.spec_decode import NgramDrafter, drafter_from_env, spec_tokens_from_env


# ------------------------------------------------------------------ drafter
def test_ngram_no_match_gives_nothing():
    d = NgramDrafter()
    assert d([1, 2, 3, 4, 5, 6], 3) == []
    assert d([], 3) == [] and d([7], 3) == [] and d([7, 7], 3) == []      # too short for a 2-gram with a successor
    assert d([1, 2, 9, 1, 2], 0) == []
    # a single repeated token is below min_n = 2
    assert d([1, 2, 3, 9, 8, 3], 3) == []


def test_ngram_longest_suffix_wins():
    #          0  1  2  3   4  5  6   7  8  9  10
    hist = [5, 1, 2, 3, 40, 9, 2, 3, 50, 1, 2, 3]
    # suffix (1, 2, 3) occurs at 1 -> 40; the shorter (2, 3) occurs later, at 6 -> 50
    assert NgramDrafter(max_n=4, min_n=2)(hist, 1) == [40]
    assert NgramDrafter(max_n=2, min_n=2)(hist, 1) == [50]


def test_ngram_most_recent_occurrence_wins():
    hist = [1, 2, 10, 0, 1, 2, 20, 0, 0, 1, 2]
    assert NgramDrafter()(hist, 2) == [20, 0]


def test_ngram_cut_at_k_and_at_the_end():
    hist = [1, 2, 3, 4, 5, 6, 1, 2]
    assert NgramDrafter()(hist, 3) == [3, 4, 5]
    assert NgramDrafter()(hist, 1) == [3]
    assert NgramDrafter()(hist, 7) == [3, 4, 5, 6, 1, 2]          # the history ends
    assert NgramDrafter()([1, 2, 1, 2], 5) == [1, 2]


def test_env_switches(monkeypatch):
    monkeypatch.delenv("LUMEN_SPEC_DECODE", raising=False)
    monkeypatch.delenv("LUMEN_SPEC_TOKENS", raising=False)
    assert drafter_from_env() is None and spec_tokens_from_env() == 3
    monkeypatch.setenv("LUMEN_SPEC_DECODE", "ngram")
    monkeypatch.setenv("LUMEN_SPEC_TOKENS", "12")
    assert isinstance(drafter_from_env(), NgramDrafter) and spec_tokens_from_env() == 7
    assert spec_tokens_from_env(0) == 1 and spec_tokens_from_env(5) == 5
    monkeypatch.setenv("LUMEN_SPEC_DECODE", "medusa")
    with pytest.raises(ValueError):
        drafter_from_env()


# ------------------------------------------------------------------ paged_verify reference
def test_paged_verify_reference_vs_dense_attention():
    H, Hkv, D, T = 6, 2, 32, 4
    G = H // Hkv
    g = torch.Generator().manual_seed(5)
    ctx = [1, 5, 64, 66, 131, 1]            # tokens in the cache including the rows
    n_rows = [1, 4, 3, 4, 2, 1]
    B, W = len(ctx), 3
    NB = 16
    kc = torch.full((NB, Hkv, 64, D), float("nan"))
    vc = torch.full((NB, Hkv, D, 64), float("nan"))
    perm = torch.randperm(NB, generator=g)
    bt = torch.zeros((B, W), dtype=torch.int32)
    ks, vs, used = [], [], 0
    for b, L in enumerate(ctx):
        k, v = torch.randn(L, Hkv, D, generator=g), torch.randn(L, Hkv, D, generator=g)
        ks.append(k)
        vs.append(v)
        for j in range(-(-L // 64)):
            blk = int(perm[used])
            used += 1
            bt[b, j] = blk
            m = min(64, L - 64 * j)
            kc[blk, :, :m, :] = k[64 * j:64 * j + m].permute(1, 0, 2)
            vc[blk, :, :, :m] = v[64 * j:64 * j + m].permute(1, 2, 0)
    q = torch.randn(B * T, (H + 2 * Hkv) * D, generator=g)
    out = lops.paged_verify(q, kc, vc, bt, torch.tensor(ctx, dtype=torch.int32),
                            torch.tensor(n_rows, dtype=torch.int32), T, H, Hkv)
    assert out.shape == (B * T, H * D) and torch.isfinite(out).all()
    for b in range(B):
        for i in range(T):
            row = out[b * T + i].view(H, D)
            if i >= n_rows[b]:
                assert (row == 0).all(), "padding rows come out zero"
                continue
            p = ctx[b] - n_rows[b] + i
            for h in range(H):
                s = (ks[b][:p + 1, h // G] @ q[b * T + i, h * D:(h + 1) * D]) / math.sqrt(D)
                want = torch.softmax(s, 0) @ vs[b][:p + 1, h // G]
                assert torch.allclose(row[h], want, atol=1e-5, rtol=1e-5), (b, i, h)
    with pytest.raises(ValueError):
        lops.paged_verify(q[:B * T - 1], kc, vc, bt, torch.tensor(ctx, dtype=torch.int32),
                          torch.tensor(n_rows, dtype=torch.int32), T, H, Hkv)
    with pytest.raises(ValueError):                                       # 24 rows x 3 heads per kv head > 64 columns
        lops.paged_verify(q, kc, vc, bt[:1], torch.tensor(ctx[:1], dtype=torch.int32),
                          torch.tensor(n_rows[:1], dtype=torch.int32), 24, H, Hkv)


# ------------------------------------------------------------------ engine
CFG = LLM_PRESETS["tiny"]
NEW = 24
SPEC = 3                      # draft tokens per step: T = 4 rows
PROMPT = [int(t) for t in np.random.default_rng(11).integers(3, CFG.vocab_size, 37)]


@pytest.fixture(scope="module")
def model():
    m = LLM(CFG, dtype=torch.float32, device="cpu")
    m.random_init(3)
    return m


def _run(m, reqs, drafter=None, spec_tokens=SPEC, stagger=False):
    """reqs: [(prompt, SamplingParams)] -> ([tokens], [finish reasons], stats)"""
    kv = PagedKVCache(CFG.num_layers, m.Hkv, CFG.head_dim, num_blocks=64, dtype=torch.float32)
    eng = LLMEngine(m, kv, lambda ids: m.embed_tokens(torch.tensor(ids)), max_batch=8, drafter=drafter,
                    spec_tokens=spec_tokens)
    try:
        rs = []
        for p, sp in reqs:
            rs.append(eng.submit(p, len(p), sp, prompt_ids=p))
            if stagger:
                next(iter(rs[-1].stream(timeout=60)))       # its first token is out before the next joins
        for r in rs:
            for _ in r.stream(timeout=60):
                pass
        return [list(r.tokens) for r in rs], [r.finish_reason for r in rs], dict(eng.stats)
    finally:
        eng.close()


@pytest.fixture(scope="module")
def truth(model):
    toks, _, st = _run(model, [(PROMPT, SamplingParams(max_new_tokens=NEW))])
    assert len(toks[0]) == NEW and st["spec_steps"] == 0 and st["decode_steps"] == NEW - 1
    return toks[0]


class Script:
    """A drafter that knows the non-speculative output: ``kind`` oracle replays it, liar proposes a
    wrong first token, half a right first and a wrong second token."""

    def __init__(self, kind, truth, prompt_len=len(PROMPT)):
        self.kind, self.truth, self.plen = kind, truth, prompt_len
        self.calls = []

    def __call__(self, token_ids, k):
        n = len(token_ids) - self.plen                # generated so far
        assert list(token_ids[:self.plen]) == PROMPT and list(token_ids[self.plen:]) == self.truth[:n]
        self.calls.append((n, k))
        t = self.truth[n:n + k]
        wrong = lambda x: (x + 1) % CFG.vocab_size  # noqa: E731
        if self.kind == "liar":
            t = [wrong(x) for x in t]
        elif self.kind == "half":
            t = t[:1] + [wrong(x) for x in t[1:2]]
        return t

    def expect(self, new=NEW, spec=SPEC):
        """(verify steps, plain steps, drafted, accepted) of a request of ``new`` tokens"""
        n, ver, plain, drafted, acc = 1, 0, 0, 0, 0    # the prefill yields token 0
        while n < new:
            k = min(spec, new - n - 1)
            d = 0 if k <= 0 else len(self(list(PROMPT) + self.truth[:n], k))
            if d == 0:
                plain += 1
                n += 1
                continue
            a = {"oracle": d, "liar": 0, "half": 1}[self.kind]
            ver, drafted, acc, n = ver + 1, drafted + d, acc + a, n + a + 1
        return ver, plain, drafted, acc


@pytest.mark.parametrize("kind", ["oracle", "liar", "half"])
def test_engine_same_tokens_under_scripted_drafters(model, truth, kind):
    ver, plain, drafted, acc = Script(kind, truth).expect()
    toks, reasons, st = _run(model, [(PROMPT, SamplingParams(max_new_tokens=NEW))], Script(kind, truth))
    assert toks[0] == truth and reasons[0] == "length"
    assert (st["spec_steps"], st["decode_steps"]) == (ver, plain)
    assert (st["spec_drafted"], st["spec_accepted"]) == (drafted, acc)
    assert st["tokens"] == NEW
    if kind == "oracle":
        assert acc == drafted > 0
        assert st["decode_steps"] + st["spec_steps"] <= -(-NEW // (SPEC + 1)) + plain
    if kind == "liar":
        assert acc == 0 and st["decode_steps"] + st["spec_steps"] == NEW - 1     # one token per step
    if kind == "half":
        # every verify step leaves a rejected row's k / v beyond ctx: the next step rewrites it
        assert acc == ver > 0 and drafted > acc


@pytest.mark.parametrize("kind", ["oracle", "liar", "half"])
def test_engine_stop_token_inside_an_accepted_run(model, truth, kind):
    idx = next(i for i in range(10, NEW) if truth[i] not in truth[:i])      # oracle: a middle row of its third step
    sp = dict(max_new_tokens=NEW, stop_token_ids=(truth[idx],))
    base, reasons, _ = _run(model, [(PROMPT, SamplingParams(**sp))])
    assert base[0] == truth[:idx] and reasons[0] == "eos_token"
    toks, reasons, st = _run(model, [(PROMPT, SamplingParams(**sp))], Script(kind, truth))
    assert toks[0] == truth[:idx] and reasons[0] == "eos_token" and st["tokens"] == idx
    assert st["spec_steps"] > 0


@pytest.mark.parametrize("kind", ["oracle", "liar", "half"])
@pytest.mark.parametrize("new", [1, 2, 3, 6])
def test_engine_never_exceeds_max_new_tokens(model, truth, kind, new):
    s = Script(kind, truth)
    toks, reasons, st = _run(model, [(PROMPT, SamplingParams(max_new_tokens=new))], s)
    assert toks[0] == truth[:new] and reasons[0] == "length" and st["tokens"] == new
    assert all(n + k + 1 <= new for n, k in s.calls)
    ver, plain, drafted, acc = Script(kind, truth).expect(new)
    assert (st["spec_steps"], st["decode_steps"], st["spec_drafted"], st["spec_accepted"]) == (ver, plain, drafted, acc)


@pytest.mark.parametrize("other", [dict(temperature=0.8, top_p=0.9, seed=1), dict(repetition_penalty=1.2)],
                         ids=["sampled", "penalised"])
def test_engine_sampled_or_penalised_batch_takes_the_existing_path(model, truth, other):
    """the other request joins first and outlasts the greedy one, so every decode step of the greedy
    request runs in a batch that may not speculate"""
    long = [int(t) for t in np.random.default_rng(12).integers(3, CFG.vocab_size, 21)]
    reqs = [(long, SamplingParams(max_new_tokens=60, **other)), (PROMPT, SamplingParams(max_new_tokens=8))]

    def drafter(token_ids, k):
        raise AssertionError("no draft may be asked for in a batch that cannot speculate")

    base, _, _ = _run(model, reqs, stagger=True)
    toks, _, st = _run(model, reqs, drafter, stagger=True)
    assert st["spec_steps"] == 0 and st["spec_drafted"] == 0
    assert toks == base and toks[1] == truth[:8] and len(toks[0]) == 60


def test_engine_two_requests_one_with_drafts(model, truth):
    """B = 2 verify steps with mixed n_rows: each request gets the tokens it gets alone"""
    other = [int(t) for t in np.random.default_rng(13).integers(3, CFG.vocab_size, 70)]
    alone, _, _ = _run(model, [(other, SamplingParams(max_new_tokens=NEW))])
    oracle = Script("oracle", truth)

    def drafter(token_ids, k):
        return oracle(token_ids, k) if list(token_ids[:len(PROMPT)]) == PROMPT else []

    toks, _, st = _run(model, [(other, SamplingParams(max_new_tokens=NEW)), (PROMPT, SamplingParams(max_new_tokens=NEW))],
                       drafter, stagger=True)
    assert toks == [alone[0], truth]
    assert st["spec_steps"] > 0 and st["spec_accepted"] == st["spec_drafted"] > 0


def test_engine_ngram_from_env(model, monkeypatch):
    """LUMEN_SPEC_DECODE=ngram on a prompt that repeats itself: drafts come from the prompt ids"""
    rep = PROMPT[:12] * 4
    monkeypatch.delenv("LUMEN_SPEC_DECODE", raising=False)
    base, _, st = _run(model, [(rep, SamplingParams(max_new_tokens=16))])
    assert st["spec_steps"] == 0
    monkeypatch.setenv("LUMEN_SPEC_DECODE", "ngram")
    monkeypatch.setenv("LUMEN_SPEC_TOKENS", "2")
    kv = PagedKVCache(CFG.num_layers, model.Hkv, CFG.head_dim, num_blocks=64, dtype=torch.float32)
    eng = LLMEngine(model, kv, lambda ids: model.embed_tokens(torch.tensor(ids)), max_batch=8)
    try:
        assert isinstance(eng.drafter, NgramDrafter) and eng.spec_T == 3
        r = eng.submit(rep, len(rep), SamplingParams(max_new_tokens=16), prompt_ids=rep)
        for _ in r.stream(timeout=60):
            pass
        assert list(r.tokens) == base[0]
        assert eng.stats["spec_drafted"] > 0
    finally:
        eng.close()
