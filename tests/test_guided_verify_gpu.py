"""Speculative decoding of guided requests on the GPU: the sampler's guided verify form
(csrc/sampler.hip) against its CPU reference, and the engine's ``verify_guided`` steps (Qwen2-0.5B,
random weights) eager and as a captured graph."""
import functools
import re

import numpy as np
import pytest
import torch

from lumen_amd import ops
from lumen_amd.models.llm import LLM, LLM_PRESETS
from lumen_amd.ops import llm as lops
from lumen_amd.runtime import guided as gd
from lumen_amd.runtime.engine import LLMEngine, SamplingParams
from lumen_amd.runtime.kv_cache import PagedKVCache

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 64
# 1,000: one launch, 31.25 bitmap words (a ragged last word).  20,481: five 4096-column chunks and a
# chunk of one column, which is also the whole last word.
SIZES = [1000, 20481]
A = 8            # grammar states of the hand-made arena
B, T = 4, 4
S = 4            # bitmap slots: 0 and 2 are owned, 1 and 3 hold junk that must stay
STATE0 = 3       # what every row of g_state holds before and after


def _logits(V, R, seed):
    """distinct by construction: per row a seeded permutation of an arithmetic sequence over [-12, 12]"""
    base = torch.linspace(-12, 12, V, dtype=torch.float64).float()
    g = torch.Generator().manual_seed(seed)
    return torch.stack([base[torch.randperm(V, generator=g)] for _ in range(R)])


def _bitmap(V, ids):
    row = np.zeros(lops.seen_words(V), np.uint32)
    for t in ids:
        row[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    return row


@functools.lru_cache(maxsize=None)
def _case(V):
    """B = 4 sequences of T = 4 rows, with the CPU reference computed once.  State a of the arena
    allows ``sets[a]``.  The inputs are built row by row from the reference's own draws, so that
    sequence 0 accepts every draft, 1 rejects its first, 2 (two live rows) accepts its one, 3 accepts
    one and rejects the next:
      0: sampled, top_p 0.9, penalty 1.3 over slot 0, all four rows in the half-vocabulary state 4;
         its draft inputs were drawn in that state, so they lie in the allowed set
      1: sampled, no penalty; rows in state 3 (exactly 64 tokens), 0 (nothing: tok = -1), 1 (one
         token, the last column), 5 (everything)
      2: unguided (g_in = -1), sampled, n_rows = 2: rows 2 and 3 are dead
      3: greedy, penalty 1.3 over slot 2; rows in states 2 (five tokens), 1, 6, a state beyond the arena"""
    R = B * T
    logits = _logits(V, R, seed=V + 1)      # a seed at which the asserts on the case itself (below) hold at both sizes
    order = logits.argsort(dim=1, descending=True)
    rng = np.random.default_rng(V + 1)
    sets = [
        set(),                                                                    # 0: allows nothing
        {V - 1},                                                                  # 1: one token, the last column
        {int(order[12, 2]), int(order[12, 9]), 0, 517, (V - 1) // 32 * 32},       # 2: five, one in the ragged word
        set(int(t) for t in rng.choice(V, 64, replace=False)),                    # 3: exactly 64
        set(int(t) for t in rng.choice(V, V // 2, replace=False)),                # 4: half
        set(range(V)),                                                            # 5: everything
        set(int(t) for t in rng.choice(V, 200, replace=False)),                   # 6
        set(int(t) for t in rng.choice(V, 7, replace=False)),                     # 7
    ]
    allow = np.stack([_bitmap(V, s) for s in sets]).view(np.int32)
    dfa = np.tile(((np.arange(A) + 1) % A).astype(np.int16)[:, None], (1, 256))
    tb = [bytes([t % 256]) for t in range(V)]
    off, dat = gd.token_csr(tb)
    cpu = dict(allow=torch.from_numpy(allow), dfa=torch.from_numpy(dfa), off=torch.from_numpy(off),
               dat=torch.from_numpy(dat.copy()))
    g_in = np.array([4, 4, 4, 4, 3, 0, 1, 5, -1, -1, -1, -1, 2, 1, 6, A + 3], np.int32)
    n_rows = [4, 4, 2, 4]
    seq = dict(inv_t=[1 / 0.8, 1 / 0.9, 1 / 0.7, 1.0], top_p=[0.9, 1.0, 0.95, 1.0], pen=[1.3, 1.0, 1.0, 1.3],
               greedy=[0, 0, 0, 1], slot=[0, -1, -1, 2])
    accept = [[True, True, True], [False, True, True], [True, True, True], [True, False, True]]
    seen = np.zeros((S, lops.seen_words(V)), np.uint32)
    seen[0] = _bitmap(V, sorted(sets[4])[:40] + [int(order[0, 0]), int(order[1, 3])])      # overlaps the allowed set
    seen[2] = _bitmap(V, sorted(sets[6])[:30] + [int(order[12, 2])])
    seen[1] = _bitmap(V, [int(t) for t in rng.choice(V, 50, replace=False)])
    seen[3] = _bitmap(V, [int(t) for t in rng.choice(V, 50, replace=False)])
    seen = torch.from_numpy(seen.view(np.int32).copy())
    state = torch.full((6,), STATE0, dtype=torch.int32)

    def ref(in_ids, u):
        g = lops.GuideTensors(cpu["allow"], cpu["dfa"], cpu["off"], cpu["dat"], [5] * B, g_in, state)
        return lops.sample_verify_rows(logits, T, n_rows, seq["inv_t"], seq["top_p"], seq["pen"], u, seq["greedy"],
                                       seq["slot"], seen.clone(), in_ids, guide=g)

    in_ids = np.array([int(order[r, 1]) for r in range(R)], np.int64)
    in_ids[0] = next(int(x) for x in order[1] if int(x) in sets[4])      # see the test: the best allowed token of row 1
    u = np.zeros(R)
    for q in range(T):
        # candidates and lse of column q depend on the inputs 0 .. q only, not on u: choose u as the
        # midpoint of a candidate's interval, draw, and make the next input from the draw
        v, i, lse, _, _, _ = ref(in_ids, u)
        for b in range(B):
            r = b * T + q
            if q >= n_rows[b]:
                continue
            fin = torch.isfinite(v[r])
            nf = int(fin.sum())
            assert bool((v[r, :nf][:-1] > v[r, :nf][1:]).all()), "transformed candidates must be distinct: change the seed"
            if seq["greedy"][b] or nf == 0:
                continue
            c = np.cumsum(np.exp(v[r].numpy().astype(np.float64) - np.float64(lse[r])))
            tp = seq["top_p"][b]
            qq = c / c[-1] if c[-1] < tp else c
            if tp < 1.0:
                assert np.abs(qq[:nf] - tp).min() >= 5e-4, (r, "top_p too close to a cumulative mass: change it")
            n = max(1, min(int(np.searchsorted(c, tp * c[-1] if c[-1] < tp else tp) + 1), K))
            cdf = c[:n] / c[n - 1]
            m = n // 2
            lo = cdf[m - 1] if m > 0 else 0.0
            assert cdf[m] - lo >= 1e-6
            u[r] = 0.5 * (lo + cdf[m])
        tok = ref(in_ids, u)[3]
        for b in range(B):
            r = b * T + q
            if q + 1 < n_rows[b]:
                t = int(tok[r])
                other = next(int(x) for x in order[r, 5:8] if int(x) != t)
                in_ids[r + 1] = t if accept[b][q] and t >= 0 else other
    out = ref(in_ids, u)
    return dict(V=V, logits=logits, sets=sets, seq=seq, n_rows=n_rows, g_in=g_in, in_ids=in_ids, u=u, seen=seen,
                cpu=cpu, ref=out)


def _device_guide(c, g_in=None):
    cpu = c["cpu"]
    return lops.GuideTensors(cpu["allow"].to(DEV), cpu["dfa"].to(DEV), cpu["off"].to(DEV), cpu["dat"].to(DEV),
                             [5] * B, c["g_in"] if g_in is None else g_in,
                             torch.full((6,), STATE0, dtype=torch.int32, device=DEV))


def _call(c, logits, seen, **kw):
    s = c["seq"]
    return lops.sample_verify_rows(logits, T, c["n_rows"], s["inv_t"], s["top_p"], s["pen"], c["u"], s["greedy"],
                                   s["slot"], seen, c["in_ids"], **kw)


@pytest.mark.parametrize("V", SIZES)
@pytest.mark.parametrize("candidates", [True, False], ids=["candidates", "tokens_only"])
def test_guided_verify_op_matches_reference(V, candidates):
    c = _case(V)
    rv, ri, rlse, rtok, racc, rseen = c["ref"]
    d_logits = c["logits"].to(DEV)
    keep = d_logits.clone()
    g = _device_guide(c)
    v, i, lse, tok, n_acc, seen = _call(c, d_logits, c["seen"].to(DEV), candidates=candidates, guide=g)
    torch.cuda.synchronize()
    assert torch.equal(d_logits, keep), "the logits are read only"
    assert torch.equal(tok.cpu(), rtok), (tok.cpu().tolist(), rtok.tolist())
    assert torch.equal(n_acc.cpu(), racc), (n_acc.cpu().tolist(), racc.tolist())
    assert torch.equal(seen.cpu(), rseen)
    assert torch.equal(seen.cpu()[[1, 3]], c["seen"][[1, 3]]), "junk rows of the bitmap are untouched"
    assert torch.equal(g.state.cpu(), torch.full((6,), STATE0, dtype=torch.int32)), "g_state is neither read nor written"
    live = torch.tensor([q < c["n_rows"][b] for b in range(B) for q in range(T)])
    if candidates:
        fin = torch.isfinite(rv) & live[:, None]
        assert torch.equal(v.cpu()[live], rv[live]), "candidate values (-inf beyond the allowed set)"
        assert torch.equal(i.cpu()[fin], ri[fin])
        assert bool((i.cpu()[live[:, None] & ~torch.isfinite(rv)] == -1).all()), "a masked column is never a candidate"
        # rtol 1e-5 is the relative bound test_kernels_gpu.py puts on row_topk's lse
        assert torch.allclose(lse.cpu()[live], rlse[live], rtol=1e-5, atol=0)
    else:
        assert v is None and i is None and lse is None
    # the reference itself: what the rows were built to show
    toks, sets, ids = rtok.tolist(), c["sets"], c["in_ids"].tolist()
    assert racc.tolist() == [3, 0, 1, 1], "all accepted; rejected at the first draft; one live draft; one of two"
    assert toks[10] == toks[11] == -1, "dead rows"
    for r, s in enumerate(c["g_in"].tolist()):
        if live[r] and 0 <= s < A and sets[s]:
            assert toks[r] in sets[s], (r, s)
    assert toks[5] == -1 and toks[15] == -1, "a state that allows nothing; a state outside the arena"
    assert toks[6] == toks[13] == V - 1, "one token, on the last column"
    assert int(torch.isfinite(rv[4]).sum()) == 64 and int(torch.isfinite(rv[12]).sum()) == 5
    assert int(torch.isfinite(rv[6]).sum()) == 1
    assert all(t in sets[4] for t in ids[1:4]), "draft inputs of sequence 0 lie in the allowed set of its later rows"
    # the last token of sequence 0 is the best allowed token of its row 1: there it is an input of an
    # earlier row (OR-ed into the staged bitmap, not in the slot) whose allow bit is set, so it is
    # penalised and no longer the best candidate -- a lost bit on either side would put it first
    best = next(int(x) for x in c["logits"][1].argsort(descending=True) if int(x) in sets[4])
    assert ids[0] == best and int(ri[1, 0]) != best


@pytest.mark.parametrize("V", SIZES)
def test_unguided_and_positional_calls_keep_their_bits(V):
    """the raw ops called positionally the pre-existing way; through ops.llm without a guide; and the
    guided verify kernels with every row unguided (g_in = -1): all the same bits"""
    c = _case(V)
    s, R = c["seq"], B * T
    d_logits = c["logits"].to(DEV)
    t = lambda x, dt: torch.as_tensor(np.asarray(x), dtype=dt, device=DEV)  # noqa: E731
    args = (t(s["inv_t"], torch.float32), t(s["top_p"], torch.float64), t(s["pen"], torch.float32),
            t(c["u"], torch.float64), t(s["greedy"], torch.int32), t(s["slot"], torch.int32))
    outs = []
    for how in ("raw", "ops", "guided_off"):
        seen = c["seen"].to(DEV)
        if how == "raw":
            tok, n_acc = torch.empty(R, dtype=torch.int32, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
            v = torch.empty((R, K), dtype=torch.float32, device=DEV)
            i = torch.empty((R, K), dtype=torch.int32, device=DEV)
            lse = torch.empty(R, dtype=torch.float32, device=DEV)
            ops.hip_ops().sample_verify_rows(d_logits, T, t(c["n_rows"], torch.int32), *args, seen,
                                             t(c["in_ids"], torch.long), tok, n_acc, v, i, lse)
        else:
            g = _device_guide(c, [-1] * R) if how == "guided_off" else None
            v, i, lse, tok, n_acc, seen = _call(c, d_logits, seen, guide=g)
            if g is not None:
                assert torch.equal(g.state.cpu(), torch.full((6,), STATE0, dtype=torch.int32))
        torch.cuda.synchronize()
        live = torch.tensor([q < c["n_rows"][b] for b in range(B) for q in range(T)])
        outs.append((v.view(torch.int32).cpu()[live], i.cpu()[live], lse.view(torch.int32).cpu()[live], tok.cpu(),
                     n_acc.cpu(), seen.cpu()))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
    # the decode form's raw positional call (14 arguments) against ops.llm without a guide
    rows = [b * T for b in range(B)]
    dec = []
    for how in ("raw", "ops"):
        seen = c["seen"].to(DEV)
        lg, u = d_logits[rows].contiguous(), t(c["u"][rows], torch.float64)
        if how == "raw":
            ids, tok = torch.empty(B, dtype=torch.long, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
            v = torch.empty((B, K), dtype=torch.float32, device=DEV)
            i = torch.empty((B, K), dtype=torch.int32, device=DEV)
            lse = torch.empty(B, dtype=torch.float32, device=DEV)
            ops.hip_ops().sample_rows(lg, args[0], args[1], args[2], u, args[4], args[5], seen,
                                      t(c["in_ids"][rows], torch.long), ids, tok, v, i, lse)
        else:
            v, i, lse, tok, seen = lops.sample_rows(lg, args[0], args[1], args[2], u, args[4], args[5], seen,
                                                    t(c["in_ids"][rows], torch.long))
        torch.cuda.synchronize()
        dec.append((v.view(torch.int32).cpu(), i.cpu(), lse.view(torch.int32).cpu(), tok.cpu(), seen.cpu()))
    for a, b in zip(*dec):
        assert torch.equal(a, b)


def test_partial_guide_arguments_are_rejected():
    """the guide tensors come all together or not at all, in the verify form too"""
    c = _case(1000)
    s, R = c["seq"], B * T
    g = _device_guide(c)
    t = lambda x, dt: torch.as_tensor(np.asarray(x), dtype=dt, device=DEV)  # noqa: E731
    with pytest.raises(RuntimeError, match="guide tensors come together"):
        ops.hip_ops().sample_verify_rows(
            c["logits"].to(DEV), T, t(c["n_rows"], torch.int32), t(s["inv_t"], torch.float32),
            t(s["top_p"], torch.float64), t(s["pen"], torch.float32), t(c["u"], torch.float64),
            t(s["greedy"], torch.int32), t(s["slot"], torch.int32), c["seen"].to(DEV), t(c["in_ids"], torch.long),
            torch.empty(R, dtype=torch.int32, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV),
            None, None, None, g.allow, g.dfa)


# ------------------------------------------------------------------ engine
CFG = LLM_PRESETS["qwen2-0.5b"]
NEW, SPEC = 24, 3
EOS = 299
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float8_e4m3fn], ids=["bf16", "fp8"])
# 300-token prompts: eager launches and the graphs' width bucket then use the same attention split
# count, and so give the same bits (see LONG in test_sample_verify_gpu.py)
LONG = [[int(t) for t in np.random.default_rng(s).integers(0, 150000, 300)] for s in (61, 62, 63, 64)]
# every byte of the runs #=# and #@ is spelled by exactly one token (asserted from the vocabulary), so
# under the mask those drafts are accepted whatever the model's logits are
PATTERN = r"#=#(yes|no|maybe)#@"
KINDS = [{}, dict(temperature=0.9, top_p=0.95, seed=11), dict(temperature=0.8, repetition_penalty=1.3, seed=5)]


def _vocab():
    multi = ["true", "false", "null", ", ", '{"', '":', '": ', '"}', "yes", "no", "maybe", "ye", "may", "be",
             '"n"', '"ok"', "10", "42", "99", "00", "07", "123", "ab", "abc", "the", " a", "tru", "e}", "€", "日本"]
    tb = [bytes([i]) for i in range(256)] + [m.encode() for m in multi]
    tb += [bytes([97 + i % 26, 97 + i // 26]) for i in range(298 - len(tb))]
    return tb + [b"", b""] + [b""] * (CFG.vocab_size - 300)


@pytest.fixture(scope="module")
def model():
    m = LLM(CFG, device=DEV)
    m.random_init(8)
    return m


@pytest.fixture(scope="module")
def guide():
    vocab = _vocab()
    for ch in b"#=@":
        spelled = [t for t, b in enumerate(vocab) if b[:1] == bytes([ch])]
        assert spelled == [ch], "the byte is spelled by its single-byte token alone"
    return vocab, gd.compile_guide("regex", PATTERN, vocab, [EOS])


def _run(m, dtype, graphs, reqs, spec_guided):
    """reqs [(prompt, SamplingParams kwargs)], all joining the batch in the same engine iteration
    -> ([tokens], [finish reasons], stats, captured graph modes)"""
    kv = PagedKVCache(CFG.num_layers, m.Hkv, CFG.head_dim, num_blocks=48, device=DEV, dtype=dtype)
    eng = LLMEngine(m, kv, lambda ids: m.embed_tokens(torch.tensor(ids, device=DEV)), max_batch=4,
                    use_graphs=graphs, spec_tokens=SPEC, spec_guided=spec_guided)
    try:
        hold, eng.max_prefill = eng.max_prefill, 0
        rs = [eng.submit(p, len(p), SamplingParams(max_new_tokens=NEW, stop_token_ids=(EOS,), **sp), prompt_ids=p)
              for p, sp in reqs]
        eng.max_prefill = hold
        for r in rs:
            for _ in r.stream(timeout=120):
                pass
        modes = sorted({k[2] for k in eng.graphs.graphs}) if eng.graphs is not None else []
        assert graphs == (eng.graphs is not None), "the graphs were dropped"
        if eng._slots is not None:
            assert sorted(eng._slots._free_slots) == list(range(4)), "a bitmap slot was not given back"
        if eng._arena is not None:
            assert sorted(eng._arena._free_slots) == list(range(4)), "a grammar-state row was not given back"
        return [list(r.tokens) for r in rs], [r.finish_reason for r in rs], dict(eng.stats), modes
    finally:
        eng.close()


def _agree(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


@DTYPES
def test_engine_guided_verify_graphs_and_eager_give_the_same_tokens(model, guide, dtype):
    vocab, g = guide
    reqs = [(LONG[k], dict(guide=g, **kw)) for k, kw in enumerate(KINDS)]
    reqs.append((LONG[3], dict(temperature=0.7, seed=2)))            # the unguided request rides along
    off, _, st_off, modes_off = _run(model, dtype, True, reqs, False)
    assert st_off["spec_steps"] == 0 and "verify_guided" not in modes_off
    eager, why_e, st_e, _ = _run(model, dtype, False, reqs, True)
    graph, why_g, st_g, modes = _run(model, dtype, True, reqs, True)
    print(f"{dtype}: graphs {st_g['spec_guided_steps']} guided verify + {st_g['decode_steps']} plain steps, forced "
          f"{st_g['spec_forced_accepted']}/{st_g['spec_forced_drafted']} accepted; speculation off: "
          f"{st_off['decode_steps']} steps")
    assert graph == eager
    assert "verify_guided" in modes, "no verify_guided graph was captured"
    head, tail = [ord("#"), ord("="), ord("#")], [ord("#"), ord("@")]
    for k in range(3):
        for toks, why in ((graph[k], why_g[k]), (off[k], "stop")):
            text = b"".join(vocab[t] for t in toks).decode()
            assert re.fullmatch(PATTERN, text), text
            assert why == "stop"
            # the forced runs are model independent: the same tokens at the same text offsets
            assert toks[:3] == head and toks[-2:] == tail
        # not asserted beyond the forced runs: a verify step rounds differently from a decode step
        print(f"request {k} {dtype}: agrees with speculation off for {_agree(graph[k], off[k])} of {len(off[k])} tokens")
    assert len(graph[3]) == NEW and why_g[3] == "length"
    for st in (st_e, st_g):
        assert st["spec_guided_steps"] > 0 and st["spec_steps"] == st["spec_guided_steps"]
        assert st["spec_forced_accepted"] >= 3 * 3, "at least = # # @ of every guided request"
        assert st["spec_sample_steps"] == 0
