"""Speculative decoding of guided requests on the CPU reference path: the grammar's forced-token
drafter (``Guide.forced``), the guided verify form of the sampler's reference
(``sample_verify_rows(guide=...)``) against the decode-form reference row by row, and the engine's
guided verify steps (``spec_guided``) against the same engine without them."""
import re

import numpy as np
import pytest
import torch

from lumen_amd.models.llm import LLM
from lumen_amd.ops import llm as lops
from lumen_amd.runtime import guided as gd
from lumen_amd.runtime.engine import LLMEngine, SamplingParams
from lumen_amd.runtime.kv_cache import PagedKVCache
from lumen_amd.runtime.spec_decode import NgramDrafter
from test_guided_engine_cpu import CFG, EOS, KINDS, PROMPTS, VOCAB, vocab300

TB = vocab300()
JSONISH = r'\{"n": [0-9]{1,3}, "ok": (true|false)\}'


def _guide(pattern, tb=TB):
    return gd.compile_guide("regex", pattern, tb, [EOS])


def _bytes(tokens, tb=TB):
    return b"".join(tb[t] for t in tokens)


# ------------------------------------------------------------------ Guide.forced
def test_forced_literal_run_stops_before_an_alternation():
    g = _guide(JSONISH)
    f = g.forced(g.start, 7)
    assert _bytes(f) == b'{"n": ', "the forced bytes up to the digit class"
    assert f == (TB.index(b'{"'), ord("n"), TB.index(b'": ')), "longest allowed token first"
    s = g.start
    for t in f:
        assert g.allows(s, t)
        s = g.walk(s, t)
    assert g.forced(s, 7) == (), "ten digits may follow: nothing is forced"
    s = g.walk(s, ord("7"))
    assert g.forced(s, 7) == (), "a digit or the comma"
    s = g.walk(g.walk(g.walk(s, ord("7")), ord("7")), ord(","))
    assert _bytes(g.forced(s, 7)) == b' "ok": ', "after the comma the run goes on to (true|false)"


def test_forced_stops_at_an_accepting_state_with_transitions():
    g = _guide(r"ab(cd)?")
    assert g.forced(g.start, 7) == (TB.index(b"ab"),), "not abc: the run ends where EOS becomes an alternative"
    s = g.walk(g.start, TB.index(b"ab"))
    assert g.accept[s] and (g.dfa[s] >= 0).sum() == 1
    assert g.forced(s, 7) == (), "an accepting state forces nothing, whatever leaves it"
    s = g.walk(s, ord("c"))
    assert g.forced(s, 7) == (ord("d"),)


def test_forced_never_yields_eos_or_a_token_without_bytes():
    for pat in (r"yes", JSONISH, r"(yes|no|maybe)", r"ab(cd)?"):
        g = _guide(pat)
        for s in range(g.n_states):
            f = g.forced(s, 7)
            assert all(TB[t] for t in f) and EOS not in f and 298 not in f, (pat, s, f)
    g = _guide(r"yes")
    assert g.forced(g.start, 7) == (TB.index(b"yes"),)
    end = g.walk(g.start, TB.index(b"yes"))
    assert g.accept[end] and g.allows(end, EOS) and g.forced(end, 7) == ()


def test_forced_k_cuts_and_the_result_is_cached():
    g = _guide(JSONISH)
    full = g.forced(g.start, 7)
    assert len(full) == 3
    for k in (0, 1, 2, 3):
        assert g.forced(g.start, k) == full[:k]
    assert g.forced(g.start, 7) == full and g.start in g._forced, "a second call answers from the cache"
    assert g.forced(-1, 3) == () and g.forced(g.n_states, 3) == ()


def test_forced_takes_the_lowest_id_among_equal_bytes():
    tb = TB + [b"yes", b'{"']                       # ids 300, 301 repeat the bytes of lower ids
    g = _guide(r"yes", tb)
    assert g.forced(g.start, 7) == (tb.index(b"yes"),) and tb.index(b"yes") < 300


# ------------------------------------------------------------------ the reference op
V, B, T = 300, 4, 4


def _op_case():
    """B = 4 sequences of T = 4 rows over the 300-id vocabulary; the arena is one compiled guide.
    Sequence 0: sampled, penalised, guided; 1: greedy, guided, two live rows; 2: unguided, sampled;
    3: greedy, penalised, guided, one row in a state outside the arena."""
    g = _guide(JSONISH)
    gen = torch.Generator().manual_seed(7)
    logits = torch.randn((B * T, V), generator=gen) * 3
    off, dat = gd.token_csr(TB)
    rng = np.random.default_rng(3)
    states = rng.integers(0, g.n_states, B * T).astype(np.int32)
    states[8:12] = -1
    states[13] = g.n_states + 5
    seen = torch.zeros((3, lops.seen_words(V)), dtype=torch.int32)
    for slot in (0, 2):
        for t in rng.choice(V, 40, replace=False):
            lops._mark_seen(seen, slot, int(t))
    c = dict(guide=g, logits=logits, n_rows=[4, 2, 3, 4], inv_t=[1 / 0.8, 1.0, 1 / 0.9, 1.0], top_p=[0.9, 1.0, 0.95, 1.0],
             pen=[1.3, 1.0, 1.0, 1.2], greedy=[0, 1, 0, 1], slot=[0, -1, -1, 2], seen=seen,
             u=rng.random(B * T), in_ids=rng.integers(0, 256, B * T), g_in=states,
             state=torch.full((5,), 3, dtype=torch.int32))
    c["tensors"] = lops.GuideTensors(torch.from_numpy(g.allow.copy()), torch.from_numpy(g.dfa.copy()),
                                     torch.from_numpy(off), torch.from_numpy(dat.copy()), [1, 2, 3, 4],
                                     [int(s) for s in states], c["state"])
    return c


def _call(c, guide):
    return lops.sample_verify_rows(c["logits"], T, c["n_rows"], c["inv_t"], c["top_p"], c["pen"], c["u"], c["greedy"],
                                   c["slot"], c["seen"].clone(), c["in_ids"], guide=guide)


def test_reference_op_is_the_decode_form_row_by_row():
    c = _op_case()
    g = c["tensors"]
    v, i, lse, tok, n_acc, seen = _call(c, g)
    assert torch.equal(c["state"], torch.full((5,), 3, dtype=torch.int32)), "state is left untouched"
    assert g.slot == [1, 2, 3, 4]
    checked = 0
    for b in range(B):
        for q in range(T):
            r = b * T + q
            if q >= c["n_rows"][b]:
                assert int(tok[r]) == -1, "a dead row"
                continue
            # the row's penalty set: the slot OR the inputs 0 .. q (the last is the call's own in_id)
            own = c["slot"][b] >= 0
            one = c["seen"][c["slot"][b]:c["slot"][b] + 1].clone() if own else c["seen"][:0]
            for t in c["in_ids"][b * T:r]:
                if own:
                    lops._mark_seen(one, 0, int(t))
            s = int(c["g_in"][r])
            gr = g._replace(slot=[0 if s >= 0 else -1], g_in=[s], state=torch.zeros(1, dtype=torch.int32))
            rv, ri, rl, rt = lops.sample_rows(c["logits"][r:r + 1], c["inv_t"][b:b + 1], c["top_p"][b:b + 1],
                                              c["pen"][b:b + 1], c["u"][r:r + 1], c["greedy"][b:b + 1],
                                              [0 if own else -1], one, c["in_ids"][r:r + 1], guide=gr)[:4]
            assert int(tok[r]) == int(rt[0]), (b, q)
            assert torch.equal(v[r], rv[0]) and torch.equal(lse[r:r + 1], rl), (b, q)
            fin = torch.isfinite(rv[0])
            assert torch.equal(i[r][fin], ri[0][fin]), (b, q)
            if 0 <= s < c["guide"].n_states:
                assert c["guide"].allows(s, int(tok[r])), "the drawn token is allowed in the row's state"
            checked += 1
    assert checked == sum(c["n_rows"])
    assert int(tok[13]) == -1, "a state outside the arena allows nothing"
    # the accept rule and the marks are the unguided form's, over the guided draws
    for b in range(B):
        j = 0
        while j < c["n_rows"][b] - 1 and int(tok[b * T + j]) == int(c["in_ids"][b * T + j + 1]):
            j += 1
        assert int(n_acc[b]) == j


def test_reference_op_with_every_row_unguided_is_the_unguided_call():
    c = _op_case()
    off = c["tensors"]._replace(g_in=[-1] * (B * T))
    a, b = _call(c, off), _call(c, None)
    for x, y in zip(a, b):
        assert torch.equal(x, y) and x.dtype == y.dtype
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
    assert torch.equal(c["state"], torch.full((5,), 3, dtype=torch.int32))


# ------------------------------------------------------------------ engine
PATTERNS = [JSONISH, r'\{"ok": (true|false), "n": [0-9]{1,2}\}', r"(yes|no|maybe)"]


@pytest.fixture(scope="module")
def model():
    m = LLM(CFG, dtype=torch.float32, device="cpu")
    m.random_init(3)
    return m


@pytest.fixture(scope="module")
def guides():
    return [gd.compile_guide("regex", p, VOCAB, [EOS]) for p in PATTERNS]


def _run(m, jobs, **kw):
    """all jobs join the batch in the same engine iteration -> (requests, stats)"""
    kv = PagedKVCache(CFG.num_layers, m.Hkv, CFG.head_dim, num_blocks=64, dtype=torch.float32)
    eng = LLMEngine(m, kv, lambda ids: m.embed_tokens(torch.tensor(ids)), max_batch=8, spec_tokens=3, **kw)
    try:
        hold, eng.max_prefill = eng.max_prefill, 0
        rs = [eng.submit(p, len(p), SamplingParams(stop_token_ids=(EOS,), **sp), prompt_ids=p) for p, sp in jobs]
        eng.max_prefill = hold
        for r in rs:
            list(r.stream(timeout=120))
        if eng._arena is not None:
            assert len(eng._arena._free_slots) == 8, "a grammar-state row was not given back"
        if eng._slots is not None:
            assert len(eng._slots._free_slots) == 8, "a bitmap slot was not given back"
        return rs, dict(eng.stats)
    finally:
        eng.close()


def _jobs(guides):
    jobs = [(PROMPTS[k], dict(max_new_tokens=40, guide=guides[k % 2], **kw)) for k, kw in enumerate(KINDS.values())]
    jobs.append((PROMPTS[3], dict(max_new_tokens=14, temperature=0.7, seed=2)))          # the unguided request
    return jobs


@pytest.fixture(scope="module")
def base(model, guides):
    rs, st = _run(model, _jobs(guides), spec_guided=False, drafter=NgramDrafter())
    return [list(r.tokens) for r in rs], st


def test_switch_off_guided_batches_take_no_verify_steps(base):
    toks, st = base
    assert st["spec_steps"] == 0 and st["spec_guided_steps"] == 0 and st["spec_forced_drafted"] == 0
    assert all(toks)


@pytest.mark.parametrize("drafter", [None, "ngram"], ids=["forced_only", "with_ngram"])
def test_engine_guided_verify_steps_give_the_same_tokens(model, guides, base, drafter):
    rs, st = _run(model, _jobs(guides), spec_guided=True, drafter=NgramDrafter() if drafter else None)
    for r, which in zip(rs[:3], (0, 1, 0)):
        text = b"".join(VOCAB[t] for t in r.tokens).decode()
        assert re.fullmatch(PATTERNS[which], text), text
        assert r.finish_reason == "stop" and EOS not in r.tokens
    assert rs[3].finish_reason == "length" and len(rs[3].tokens) == 14
    assert [list(r.tokens) for r in rs] == base[0], "speculation changed the tokens"
    assert st["spec_guided_steps"] > 0 and st["spec_steps"] == st["spec_guided_steps"]
    assert st["spec_forced_accepted"] > 0 and st["spec_forced_drafted"] >= st["spec_forced_accepted"]
    assert st["spec_drafted"] >= st["spec_forced_drafted"] and st["spec_accepted"] >= st["spec_forced_accepted"]
    assert st["spec_sample_steps"] == 0 and st["guided_steps"] == 0


@pytest.mark.parametrize("kind", list(KINDS))
def test_max_new_tokens_inside_a_forced_run(model, guides, kind):
    g = guides[0]
    for n in (2, 3, 4):              # the text starts {"n":  -- a forced run of three tokens
        rs, st = _run(model, [(PROMPTS[1], dict(max_new_tokens=n, guide=g, **KINDS[kind]))], spec_guided=True)
        r = rs[0]
        assert r.finish_reason == "length" and len(r.tokens) == n
        s = g.start
        for t in r.tokens:
            s = g.walk(s, t)
            assert s >= 0
        assert s == r.gstate


def test_choice_guide_and_env_switch(model, guides, monkeypatch):
    """(yes|no|maybe): nothing is forced at the start, the tail of a choice is; the switch from the
    environment, and the forced drafter alone"""
    monkeypatch.setenv("LUMEN_SPEC_GUIDED", "1")
    jobs = [(PROMPTS[0], dict(max_new_tokens=8, guide=guides[2], **KINDS["sampled"]))]
    rs, st = _run(model, jobs)
    monkeypatch.delenv("LUMEN_SPEC_GUIDED")
    off, st_off = _run(model, jobs)
    assert st_off["spec_steps"] == 0
    assert list(rs[0].tokens) == list(off[0].tokens) and rs[0].finish_reason == "stop"
    assert re.fullmatch(PATTERNS[2], b"".join(VOCAB[t] for t in rs[0].tokens).decode())
