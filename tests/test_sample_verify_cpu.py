"""Speculative decoding of sampled and penalised requests on the CPU reference path: the verify
form of the device sampler's reference (ops.llm.sample_verify_rows) against the existing
sample_rows run row by row, and the engine's sampled verify step under scripted drafters -- with
the same seed a request gets the tokens it gets with speculation off."""
import functools

import numpy as np
import pytest
import torch

from lumen_amd.models.llm import LLM, LLM_PRESETS
from lumen_amd.ops import llm as lops
from lumen_amd.runtime.engine import LLMEngine, SamplingParams
from lumen_amd.runtime.kv_cache import PagedKVCache

K = 64


# ------------------------------------------------------------------ the op: cases shared with the GPU test
def _logits(V, R, seed):
    """distinct by construction: per row a seeded permutation of an arithmetic sequence over [-12, 12]"""
    base = torch.linspace(-12, 12, V, dtype=torch.float64).float()
    g = torch.Generator().manual_seed(seed)
    return torch.stack([base[torch.randperm(V, generator=g)] for _ in range(R)])


def _bitmap(S, V, sets, junk_rows=()):
    seen = np.zeros((S, lops.seen_words(V)), np.uint32)
    for slot, toks in sets.items():
        for t in toks:
            seen[slot, t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    g = np.random.default_rng(V)
    for r in junk_rows:     # a slot no sequence of the launch uses: must come back untouched
        seen[r] = g.integers(0, 2 ** 32, seen.shape[1], dtype=np.uint32)
        if V % 32:
            seen[r, -1] &= np.uint32((1 << (V % 32)) - 1)
    return torch.from_numpy(seen.view(np.int32).copy())


def single_row(run, logits_row, sq, u, penalised, in_id, V):
    """the existing ``sample_rows`` (``run``: the CPU reference or the HIP op) on one row whose bitmap
    slot holds ``penalised``; -> (v [64], i [64], lse, tok)"""
    d = logits_row.device
    seen = _bitmap(1, V, {0: penalised}).to(d)
    v, i, lse, tok, _ = run(logits_row[None], [sq["inv_t"]], [sq["top_p"]], [sq["pen"]], [u], [sq["greedy"]],
                            [0 if sq["slot"] >= 0 else -1], seen, [in_id])
    return v[0].cpu(), i[0].cpu(), float(lse[0]), int(tok[0])


def _clear_of_edges(v, lse, top_p, u):
    """the nucleus cut and the pick sit at least 1e-9 off every cumulative mass, so a last-bit
    difference of exp() between two implementations cannot move either"""
    c = np.cumsum(np.exp(v.numpy().astype(np.float64) - np.float64(lse)))
    thr = top_p * c[-1] if c[-1] < top_p else top_p
    n = max(1, min(int(np.searchsorted(c, thr) + 1), K))
    return np.abs(c - thr).min() >= 1e-9 and np.abs(c[:n] / c[n - 1] - u).min() >= 1e-9


# Every sequence: n live rows, the sampling parameters, its slot, `accept` leading draft tokens that
# are made equal to the token of the row before them, and for the others `wrong`, one entry per draft
# position: an id, "seen" (a token of the slot's bitmap), "repeat" (the input before it) or "top"
# (the best logit of the row it is fed to -- a token whose penalty shows in that row's candidates).
def _seqs(name, V):
    hi = [4095, 4096] if V > 4097 else [V // 2, V // 2 + 1]        # the columns either side of the first chunk edge
    if name == "A":   # B = 3, T = 4, n_rows = [4, 1, 3]: a full, no and a partial acceptance
        return 4, [
            dict(n=4, greedy=1, inv_t=1.0, top_p=1.0, pen=1.3, slot=1, accept=3, wrong=[None] * 3),
            dict(n=1, greedy=0, inv_t=1 / 0.8, top_p=0.9, pen=1.2, slot=0, accept=0, wrong=[]),
            dict(n=3, greedy=0, inv_t=1 / 0.7, top_p=0.95, pen=1.3, slot=-1, accept=1, wrong=[None, "top"]),
        ]
    if name == "B":   # the same shape: an acceptance of 0 with a repeated draft token, rejected tokens in the bitmap
        return 4, [
            dict(n=4, greedy=0, inv_t=1 / 0.8, top_p=0.9, pen=1.2, slot=1, accept=0, wrong=["seen", "top", "repeat"]),
            dict(n=1, greedy=1, inv_t=1.0, top_p=1.0, pen=1.3, slot=-1, accept=0, wrong=[]),
            dict(n=3, greedy=1, inv_t=1.0, top_p=1.0, pen=1.3, slot=2, accept=1, wrong=[None, "seen"]),
        ]
    assert name == "C"   # B = 4, T = 8: 32 rows, draft tokens at the chunk edge, every kind of acceptance
    return 8, [
        dict(n=8, greedy=0, inv_t=1 / 0.9, top_p=0.9, pen=1.1, slot=2, accept=7, wrong=[None] * 7),
        dict(n=8, greedy=1, inv_t=1.0, top_p=1.0, pen=1.3, slot=0, accept=0,
             wrong=[hi[0], hi[1], "top", "repeat", "seen", hi[0], "top"]),
        dict(n=1, greedy=0, inv_t=1 / 0.8, top_p=0.95, pen=1.2, slot=-1, accept=0, wrong=[]),
        dict(n=5, greedy=0, inv_t=1 / 0.8, top_p=0.9, pen=1.3, slot=1, accept=2, wrong=[None, None, hi[1], "top"]),
    ]


S_SLOTS, JUNK = 4, 3


@functools.lru_cache(maxsize=None)
def build_case(V, name):
    """inputs of one launch and what the existing CPU ``sample_rows`` gives for every live row when
    it is handed the row alone with a bitmap of ``seen[slot] | {x_0 .. x_(i-1)}`` and ``in_id = x_i``"""
    T, seqs = _seqs(name, V)
    B, R = len(seqs), len(seqs) * T
    logits = _logits(V, R, seed=V + T)
    if V > 4097:      # the chunk-edge columns hold the 5th and 6th best logit of every row: penalising them shows
        top = logits.topk(6, dim=1).indices
        for r in range(R):
            for col, rank in ((4095, 4), (4096, 5)):
                o = int(top[r, rank])
                logits[r, [col, o]] = logits[r, [o, col]]
    order = logits.topk(8, dim=1).indices                            # order[r, j]: the j-th best column of row r
    low = (-logits).topk(8, dim=1).indices                           # ... and the j-th worst (a negative logit)
    sets = {sq["slot"]: {int(order[b * T, 0]), int(order[b * T, 6]), int(low[b * T, 6]), 0, V - 1}
            for b, sq in enumerate(seqs) if sq["slot"] >= 0}
    seen = _bitmap(S_SLOTS, V, sets, junk_rows=(JUNK,))
    g = np.random.default_rng(V + T)
    u = g.random(R)
    in_ids = np.full(R, 7, np.int64)           # dead rows' inputs are never read
    want = {"v": torch.full((R, K), float("nan")), "i": torch.full((R, K), -2, dtype=torch.int32),
            "lse": torch.zeros(R), "tok": torch.full((R,), -1, dtype=torch.int32),
            "n_acc": torch.tensor([sq["accept"] for sq in seqs], dtype=torch.int32), "live": []}
    after = {k: set(v) for k, v in sets.items()}
    for b, sq in enumerate(seqs):
        old = sets.get(sq["slot"], set())
        x = [int(order[b * T, 3])]                                   # the sequence's last token
        for q in range(sq["n"]):
            r = b * T + q
            v, i, lse, tok = single_row(lops.sample_rows, logits[r], sq, u[r], old | set(x[:q]), x[q], V)
            assert bool((v[:-1] > v[1:]).all()), "the candidates must be distinct: change the seed"
            assert sq["greedy"] or _clear_of_edges(v, lse, sq["top_p"], u[r]), "u or top_p on an edge: change the seed"
            want["v"][r], want["i"][r], want["lse"][r], want["tok"][r] = v, i, lse, tok
            want["live"].append(r)
            if q + 1 < sq["n"]:
                w = sq["wrong"][q]
                if q < sq["accept"]:
                    nxt = tok
                elif w == "seen":
                    nxt = sorted(old)[1]
                elif w == "repeat":
                    nxt = x[q]
                elif w == "top":
                    nxt = int(order[r + 1, 0])
                else:
                    nxt = int(w)
                assert (nxt == tok) == (q < sq["accept"]), "a draft token meant to be rejected was drawn"
                x.append(nxt)
        in_ids[b * T:b * T + sq["n"]] = x
        if sq["slot"] >= 0:
            after[sq["slot"]] |= set(x[:sq["accept"] + 1])
    want["seen"] = _bitmap(S_SLOTS, V, after, junk_rows=(JUNK,))
    return {"T": T, "B": B, "seqs": seqs, "logits": logits, "u": u, "in_ids": in_ids, "seen": seen, "sets": sets,
            "want": want}


def call_op(c, logits, seen, candidates=True):
    sq = c["seqs"]
    return lops.sample_verify_rows(logits, c["T"], [s["n"] for s in sq], [s["inv_t"] for s in sq],
                                   [s["top_p"] for s in sq], [s["pen"] for s in sq], c["u"], [s["greedy"] for s in sq],
                                   [s["slot"] for s in sq], seen, c["in_ids"], candidates=candidates)


def check_against(c, out, lse_exact=True):
    """every live row equals the one-row composition; dead rows give -1; n_acc and the bitmap"""
    v, i, lse, tok, n_acc, seen = (t.cpu() for t in out)
    w = c["want"]
    live = w["live"]
    assert torch.equal(v[live], w["v"][live])
    assert torch.equal(i[live], w["i"][live])
    if lse_exact:
        assert torch.equal(lse[live], w["lse"][live])
    else:   # rtol 1e-5 is the relative bound test_kernels_gpu.py puts on row_topk's lse
        assert torch.allclose(lse[live], w["lse"][live], rtol=1e-5, atol=0)
    assert torch.equal(tok, w["tok"]), "tokens (dead rows: -1)"
    dead = sorted(set(range(len(tok))) - set(live))
    assert dead and bool((tok[dead] == -1).all())
    assert torch.equal(n_acc, w["n_acc"])
    assert torch.equal(seen, w["seen"]), "the bitmap is old | {x_0 .. x_n_acc}; the junk slot is untouched"
    assert torch.equal(seen[JUNK], c["seen"][JUNK]) and not torch.equal(seen, c["seen"])


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_reference_is_the_row_by_row_composition(name):
    c = build_case(1000, name)
    keep = c["logits"].clone()
    out = call_op(c, c["logits"], c["seen"].clone())
    assert torch.equal(c["logits"], keep), "the logits are read only"
    check_against(c, out)
    assert out[3].dtype == torch.int32 and out[4].dtype == torch.int32
    assert sorted(int(a) for a in c["want"]["n_acc"]) == {"A": [0, 1, 3], "B": [0, 0, 1], "C": [0, 0, 2, 7]}[name]


def test_later_inputs_do_not_leak_into_a_row():
    """case A, sequence 0 (greedy, penalty 1.3, every draft accepted): row i's winner is row i + 1's
    input, and penalising it in row i as well would change row i's winner"""
    c = build_case(1000, "A")
    sq, T, V = c["seqs"][0], c["T"], 1000
    x = [int(t) for t in c["in_ids"][:sq["n"]]]
    for q in range(sq["n"] - 1):
        tok = int(c["want"]["tok"][q])
        assert x[q + 1] == tok
        leaked = single_row(lops.sample_rows, c["logits"][q], sq, 0.0, c["sets"][sq["slot"]] | set(x[:q + 2]), x[q], V)
        assert leaked[3] != tok


def test_draft_tokens_in_the_bitmap_and_repeated():
    c = build_case(1000, "B")
    x = [int(t) for t in c["in_ids"][:4]]
    assert x[1] in c["sets"][1] and x[3] == x[2], "a draft token that is already in the bitmap; a repeated one"
    assert c["seqs"][2]["slot"] == 2 and int(c["in_ids"][2 * 4 + 2]) in c["sets"][2]
    assert any(s["slot"] == -1 and s["n"] > 1 for s in build_case(1000, "A")["seqs"]), "a sequence without a slot"


def test_slot_beyond_the_bitmap_is_no_slot():
    c = build_case(1000, "A")
    seqs = [dict(s, slot=-1 if s["slot"] < 0 else s["slot"] + 10) for s in c["seqs"]]
    none = [dict(s, slot=-1) for s in c["seqs"]]
    a = call_op(dict(c, seqs=seqs), c["logits"], c["seen"].clone())
    b = call_op(dict(c, seqs=none), c["logits"], c["seen"].clone())
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and torch.equal(a[5], c["seen"])


def test_value_errors():
    c = build_case(1000, "A")
    sq = c["seqs"]
    args = lambda: ([s["n"] for s in sq], [s["inv_t"] for s in sq], [s["top_p"] for s in sq],  # noqa: E731
                    [s["pen"] for s in sq], c["u"], [s["greedy"] for s in sq], [s["slot"] for s in sq],
                    c["seen"].clone(), c["in_ids"])
    with pytest.raises(ValueError):
        lops.sample_verify_rows(c["logits"][:, :63], 4, *args())            # V < 64
    with pytest.raises(ValueError):
        lops.sample_verify_rows(c["logits"][:11], 4, *args())               # R != B * T
    with pytest.raises(ValueError):
        lops.sample_verify_rows(c["logits"], 3, *args())                    # R != B * T
    for T in (0, 9):
        with pytest.raises(ValueError):
            lops.sample_verify_rows(c["logits"][:3 * T], T, *args())        # T outside 1 .. 8


# ------------------------------------------------------------------ engine
CFG = LLM_PRESETS["tiny"]
NEW = 24
SPEC = 3                      # draft tokens per step: T = 4 rows
PROMPT = [int(t) for t in np.random.default_rng(11).integers(3, CFG.vocab_size, 37)]      # test_spec_decode_cpu's
# fp32 verify and decode logits differ by about 1e-6, so a draw within that of a cumulative-mass
# edge could differ between the runs: seed 1 sits on none (a seed that did would be replaced).
SAMPLED = dict(temperature=0.8, top_p=0.9, seed=1)
PENALISED = dict(repetition_penalty=1.3)
BOTH = dict(temperature=0.8, top_p=0.9, seed=1, repetition_penalty=1.3)
JOBS = pytest.mark.parametrize("job", [SAMPLED, PENALISED, BOTH], ids=["sampled", "penalised", "both"])
KINDS = pytest.mark.parametrize("kind", ["oracle", "liar", "half"])


@pytest.fixture(scope="module")
def model():
    m = LLM(CFG, dtype=torch.float32, device="cpu")
    m.random_init(3)
    return m


def _run(m, reqs, drafter=None, spec_sampling=True, stagger=False):
    """reqs: [(prompt, SamplingParams kwargs)] -> ([tokens], [finish reasons], stats)"""
    kv = PagedKVCache(CFG.num_layers, m.Hkv, CFG.head_dim, num_blocks=64, dtype=torch.float32)
    eng = LLMEngine(m, kv, lambda ids: m.embed_tokens(torch.tensor(ids)), max_batch=8, drafter=drafter,
                    spec_tokens=SPEC, spec_sampling=spec_sampling)
    try:
        rs = []
        for p, sp in reqs:
            rs.append(eng.submit(p, len(p), SamplingParams(**sp), prompt_ids=p))
            if stagger:
                next(iter(rs[-1].stream(timeout=60)))       # its first token is out before the next joins
        for r in rs:
            for _ in r.stream(timeout=60):
                pass
        assert eng._slots is None or sorted(eng._slots._free_slots) == list(range(8)), "a bitmap slot leaked"
        return [list(r.tokens) for r in rs], [r.finish_reason for r in rs], dict(eng.stats)
    finally:
        eng.close()


class Script:
    """A drafter that knows the non-speculative output of some prompts: ``kind`` oracle replays it,
    liar proposes a wrong first token, half a right first and a wrong second token."""

    def __init__(self, kind, truths):
        self.kind, self.truths = kind, truths          # [(prompt, tokens)]
        self.calls = []

    def __call__(self, token_ids, k):
        for p, truth in self.truths:
            if list(token_ids[:len(p)]) == p:
                break
        else:
            return []
        n = len(token_ids) - len(p)                     # generated so far
        assert list(token_ids[len(p):]) == truth[:n], "the request left the tokens of its run without speculation"
        self.calls.append((n, k))
        t = truth[n:n + k]
        wrong = lambda x: (x + 1) % CFG.vocab_size  # noqa: E731
        if self.kind == "liar":
            t = [wrong(x) for x in t]
        elif self.kind == "half":
            t = t[:1] + [wrong(x) for x in t[1:2]]
        return t

    def expect(self, new):
        """(verify steps, plain steps, drafted, accepted) of the one request of ``new`` tokens"""
        (p, truth), = self.truths
        n, ver, plain, drafted, acc = 1, 0, 0, 0, 0    # the prefill yields token 0
        while n < new:
            k = min(SPEC, new - n - 1)
            d = 0 if k <= 0 else len(Script(self.kind, self.truths)(list(p) + truth[:n], k))
            if d == 0:
                plain += 1
                n += 1
                continue
            a = {"oracle": d, "liar": 0, "half": 1}[self.kind]
            ver, drafted, acc, n = ver + 1, drafted + d, acc + a, n + a + 1
        return ver, plain, drafted, acc


@pytest.fixture(scope="module")
def truths(model):
    """the run without speculation of every job, computed once"""
    out = {}
    for name, job in (("sampled", SAMPLED), ("penalised", PENALISED), ("both", BOTH)):
        toks, reasons, st = _run(model, [(PROMPT, dict(max_new_tokens=NEW, **job))], spec_sampling=False)
        assert len(toks[0]) == NEW and st["spec_steps"] == 0 and st["decode_steps"] == NEW - 1
        out[name] = toks[0]
    return out


def _name(job):
    return "both" if job is BOTH else "sampled" if job is SAMPLED else "penalised"


@KINDS
@JOBS
def test_engine_same_tokens_as_without_speculation(model, truths, job, kind):
    truth = truths[_name(job)]
    s = Script(kind, [(PROMPT, truth)])
    ver, plain, drafted, acc = s.expect(NEW)
    toks, reasons, st = _run(model, [(PROMPT, dict(max_new_tokens=NEW, **job))], s)
    assert toks[0] == truth and reasons[0] == "length" and st["tokens"] == NEW
    assert st["spec_sample_steps"] == st["spec_steps"] == ver > 0
    assert (st["decode_steps"], st["spec_drafted"], st["spec_accepted"]) == (plain, drafted, acc)
    if kind == "oracle":
        assert acc == drafted > 0
    if kind == "liar":
        assert acc == 0 and st["decode_steps"] + st["spec_steps"] == NEW - 1     # one token per step
    if kind == "half":
        assert acc == ver and drafted > acc                                      # one per step


def test_the_jobs_differ(truths):
    """the penalty and the temperature are live: the three jobs are three different token sequences"""
    assert len({tuple(t) for t in truths.values()}) == 3


@KINDS
def test_engine_mixed_batch_with_staggered_joins(model, kind):
    """greedy, sampled, penalised and sampled + penalised requests in one batch: each request gets the
    tokens of the same batch without speculation"""
    ps = [[int(t) for t in np.random.default_rng(s).integers(3, CFG.vocab_size, n)] for s, n in ((21, 70), (22, 21), (23, 33))]
    reqs = [(ps[0], dict(max_new_tokens=40)), (PROMPT, dict(max_new_tokens=NEW, **SAMPLED)),
            (ps[1], dict(max_new_tokens=30, **PENALISED)), (ps[2], dict(max_new_tokens=NEW, **BOTH))]
    base, _, st0 = _run(model, reqs, spec_sampling=False, stagger=True)
    assert st0["spec_steps"] == 0
    s = Script(kind, [(p, t) for (p, _), t in zip(reqs, base)])
    toks, _, st = _run(model, reqs, s, stagger=True)
    assert toks == base
    assert st["spec_sample_steps"] > 0 and st["spec_drafted"] > 0
    assert (st["spec_accepted"] == st["spec_drafted"]) if kind == "oracle" else (st["spec_accepted"] < st["spec_drafted"])
    if kind == "liar":
        assert st["spec_accepted"] == 0


@KINDS
def test_engine_stop_token_inside_an_accepted_run(model, truths, kind):
    truth = truths["both"]
    idx = next(i for i in range(10, NEW) if truth[i] not in truth[:i])      # oracle: a middle row of its third step
    sp = dict(max_new_tokens=NEW, stop_token_ids=(truth[idx],), **BOTH)
    base, reasons, _ = _run(model, [(PROMPT, sp)], spec_sampling=False)
    assert base[0] == truth[:idx] and reasons[0] == "eos_token"
    toks, reasons, st = _run(model, [(PROMPT, sp)], Script(kind, [(PROMPT, truth)]))
    assert toks[0] == truth[:idx] and reasons[0] == "eos_token" and st["tokens"] == idx
    assert st["spec_sample_steps"] > 0


@KINDS
@pytest.mark.parametrize("new", [1, 2, 3, 6])
def test_engine_never_exceeds_max_new_tokens(model, truths, kind, new):
    truth = truths["both"]
    s = Script(kind, [(PROMPT, truth)])
    toks, reasons, st = _run(model, [(PROMPT, dict(max_new_tokens=new, **BOTH))], s)
    assert toks[0] == truth[:new] and reasons[0] == "length" and st["tokens"] == new
    assert all(n + k + 1 <= new for n, k in s.calls)
    ver, plain, drafted, acc = Script(kind, [(PROMPT, truth)]).expect(new)
    assert (st["spec_steps"], st["decode_steps"], st["spec_drafted"], st["spec_accepted"]) == (ver, plain, drafted, acc)
    assert st["spec_sample_steps"] == ver


@JOBS
def test_switch_off_never_asks_the_drafter(model, truths, job, monkeypatch):
    """today's behaviour: without the switch a sampled or penalised batch does not speculate"""
    def drafter(token_ids, k):
        raise AssertionError("no draft may be asked for in a batch that cannot speculate")

    monkeypatch.delenv("LUMEN_SPEC_SAMPLING", raising=False)
    for off in (False, None):
        toks, _, st = _run(model, [(PROMPT, dict(max_new_tokens=NEW, **job))], drafter, spec_sampling=off)
        assert toks[0] == truths[_name(job)] and st["spec_steps"] == 0 and st["spec_sample_steps"] == 0


def test_switch_from_env(model, monkeypatch):
    kv = PagedKVCache(CFG.num_layers, model.Hkv, CFG.head_dim, num_blocks=8, dtype=torch.float32)
    for val, want in ((None, False), ("0", False), ("1", True)):
        if val is None:
            monkeypatch.delenv("LUMEN_SPEC_SAMPLING", raising=False)
        else:
            monkeypatch.setenv("LUMEN_SPEC_SAMPLING", val)
        eng = LLMEngine(model, kv, lambda ids: model.embed_tokens(torch.tensor(ids)), max_batch=2)
        try:
            assert eng.spec_sampling is want
        finally:
            eng.close()
