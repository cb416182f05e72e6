"""The device sampler's guided form (csrc/sampler.hip) against its CPU reference, and guided requests
through the engine's ``guided`` graphs (look-ahead included) against the host sampling path."""
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
E_ID = 300       # the end-of-sequence id: a token without bytes


def _logits(V, B, seed):
    """distinct by construction: per row a seeded permutation of an arithmetic sequence over [-12, 12]"""
    base = torch.linspace(-12, 12, V, dtype=torch.float64).float()
    g = torch.Generator().manual_seed(seed)
    return torch.stack([base[torch.randperm(V, generator=g)] for _ in range(B)])


def _token_bytes(V):
    """ids 0 .. 255: the single bytes; E_ID: no bytes; the others two to four bytes"""
    tb = [bytes([t]) if t < 256 else bytes([65 + (t + k) % 26 for k in range(2 + t % 3)]) for t in range(V)]
    tb[E_ID] = b""
    return tb


def _bitmap(V, ids):
    row = np.zeros(lops.seen_words(V), np.uint32)
    for t in ids:
        row[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    return row


@functools.lru_cache(maxsize=None)
def _case(V):
    """the rows of the issue, each as a greedy and as a sampled row (16 rows), with the CPU reference
    computed once.  State a of the arena allows ``sets[a]``; every byte leads from state a to state
    (a + 1) % A, so a token of n bytes advances the state by n."""
    B = 16
    logits = _logits(V, B, seed=V + 1)
    order = logits.argsort(dim=1, descending=True)
    rng = np.random.default_rng(V)
    last_word = list(range((V - 1) // 32 * 32, V))
    rank_e = int((order[14] == E_ID).nonzero()[0, 0])
    sets = [
        set(),                                                                    # 0: allows nothing
        {V - 1},                                                                  # 1: one token, the last column
        {int(order[4, 2]), int(order[4, 9]), 0, 517, last_word[-1]},              # 2: five, one in the ragged word
        set(int(t) for t in rng.choice(V, 64, replace=False)),                    # 3: exactly 64
        set(int(t) for t in rng.choice(V, V // 2, replace=False)),                # 4: about half
        set(range(V)),                                                            # 5: everything
        {E_ID} | set(int(t) for t in order[14, rank_e + 1:rank_e + 5]),           # 6: EOS is the best allowed token
        set(int(t) for t in rng.choice(V, 200, replace=False)),                   # 7: read through g_state
    ]
    tb = _token_bytes(V)
    allow = np.stack([_bitmap(V, s) for s in sets]).view(np.int32)
    dfa = np.tile(((np.arange(A) + 1) % A).astype(np.int16)[:, None], (1, 256))
    accept = np.zeros(A, bool)
    accept[6] = True
    guide = gd.Guide("regex", "", dfa, accept, allow, tb, [E_ID])
    # case c = rows 2c (greedy) and 2c + 1 (sampled): the state it draws in (-1: an unguided row).  The
    # last case feeds g_in = -1 and reads the state preset in g_state: 6 (greedy: EOS is the best
    # allowed token) and 7 (sampled).  Every other row finds 3 in its g_state row and must not read it.
    states = [-1, 1, 2, 3, 4, 5, 0, None]
    rows = []
    state0 = np.full(B, 3, np.int32)
    for c, state in enumerate(states):
        for greedy in (1, 0):
            b = len(rows)
            pen = 1.3 if state == 4 else 1.0
            rows.append(dict(greedy=greedy, inv_t=1.0 if greedy else 1 / 0.8, top_p=1.0 if greedy or c % 2 else 0.9,
                             pen=pen, seen_slot=b if pen != 1.0 else -1, in_id=int(order[b, 1]),
                             g_slot=-1 if state == -1 else b, g_in=-1 if state is None else state))
            if state is None:
                state0[b] = 6 if greedy else 7
    seen = np.zeros((B, lops.seen_words(V)), np.uint32)
    for b, r in enumerate(rows):                      # seen bits that overlap the allowed set
        if r["seen_slot"] >= 0:
            some = sorted(sets[4])[:40] + [int(order[b, 0]), int(order[b, 3])]
            seen[b] = _bitmap(V, some)
    seen = torch.from_numpy(seen.view(np.int32).copy())
    off, dat = gd.token_csr(tb)
    cpu = dict(allow=torch.from_numpy(allow), dfa=torch.from_numpy(dfa), off=torch.from_numpy(off),
               dat=torch.from_numpy(dat.copy()))

    def ref(u):
        g = lops.GuideTensors(cpu["allow"], cpu["dfa"], cpu["off"], cpu["dat"], [r["g_slot"] for r in rows],
                              [r["g_in"] for r in rows], torch.from_numpy(state0.copy()))
        return lops.sample_rows(logits, [r["inv_t"] for r in rows], [r["top_p"] for r in rows],
                                [r["pen"] for r in rows], u, [r["greedy"] for r in rows],
                                [r["seen_slot"] for r in rows], seen.clone(), [r["in_id"] for r in rows], guide=g)

    # pass 1: candidates and lse do not depend on u; then u = the midpoint of a candidate's interval
    v, i, lse, _, _, _ = ref([0.0] * B)
    u = [0.0] * B
    for b, r in enumerate(rows):
        fin = torch.isfinite(v[b])
        nf = int(fin.sum())
        assert bool((v[b, :nf][:-1] > v[b, :nf][1:]).all()), "transformed candidates must be distinct: change the seed"
        if r["greedy"] or nf == 0:
            continue
        c = np.cumsum(np.exp(v[b].numpy().astype(np.float64) - np.float64(lse[b])))
        tp = r["top_p"]
        q = c / c[-1] if c[-1] < tp else c
        if tp < 1.0:
            assert np.abs(q[:nf] - tp).min() >= 5e-4, (b, "top_p too close to a cumulative mass: change it")
        n = max(1, min(int(np.searchsorted(c, tp * c[-1] if c[-1] < tp else tp) + 1), K))
        cdf = c[:n] / c[n - 1]
        m = n // 2
        lo = cdf[m - 1] if m > 0 else 0.0
        assert cdf[m] - lo >= 1e-6
        u[b] = 0.5 * (lo + cdf[m])
    out = ref(u)
    return dict(logits=logits, rows=rows, sets=sets, guide=guide, seen=seen, state0=state0, u=u, ref=out, cpu=cpu)


def _device_guide(c, rows):
    cpu = c["cpu"]
    return lops.GuideTensors(cpu["allow"].to(DEV), cpu["dfa"].to(DEV), cpu["off"].to(DEV), cpu["dat"].to(DEV),
                             [r["g_slot"] for r in rows], [r["g_in"] for r in rows],
                             torch.from_numpy(c["state0"].copy()).to(DEV))


@pytest.mark.parametrize("V", SIZES)
@pytest.mark.parametrize("candidates", [True, False], ids=["candidates", "tokens_only"])
def test_guided_op_matches_reference(V, candidates):
    c = _case(V)
    rows, u = c["rows"], c["u"]
    rv, ri, rlse, rtok, rseen, rstate = c["ref"]
    d_logits = c["logits"].to(DEV)
    keep = d_logits.clone()
    out_ids = torch.full((len(rows),), -7, dtype=torch.long, device=DEV)
    v, i, lse, tok, seen2, state = lops.sample_rows(
        d_logits, [r["inv_t"] for r in rows], [r["top_p"] for r in rows], [r["pen"] for r in rows], u,
        [r["greedy"] for r in rows], [r["seen_slot"] for r in rows], c["seen"].to(DEV), [r["in_id"] for r in rows],
        out_ids=out_ids, candidates=candidates, guide=_device_guide(c, rows))
    torch.cuda.synchronize()
    assert torch.equal(d_logits, keep), "the logits are read only"
    assert torch.equal(tok.cpu(), rtok), (tok.cpu().tolist(), rtok.tolist())
    assert torch.equal(out_ids.cpu(), rtok.long().clamp(min=0))
    assert torch.equal(seen2.cpu(), rseen)
    assert torch.equal(state.cpu(), rstate)
    if candidates:
        fin = torch.isfinite(rv)
        assert torch.equal(v.cpu(), rv), "candidate values (-inf beyond the allowed set)"
        assert torch.equal(i.cpu()[fin], ri[fin])
        assert bool((i.cpu()[~fin] == -1).all()), "a masked column is never a candidate"
        # rtol 1e-5 is the relative bound test_kernels_gpu.py puts on row_topk's lse
        assert torch.allclose(lse.cpu(), rlse, rtol=1e-5, atol=0)
    # the reference itself: what the rows were built to show
    g, sets, toks = c["guide"], c["sets"], rtok.tolist()
    for b, r in enumerate(rows):
        s = r["g_in"] if r["g_in"] >= 0 else int(c["state0"][b])
        if r["g_slot"] < 0:
            assert int(rstate[b]) == int(c["state0"][b]), "an unguided row owns no state"
            continue
        if not sets[s]:
            assert toks[b] == -1 and int(rstate[b]) == s, "nothing allowed: tok = -1 and the state stays"
            continue
        assert toks[b] in sets[s]
        assert int(rstate[b]) == g.walk(s, toks[b]), "g_state after the call is the host walk"
    assert toks[2] == toks[3] == V - 1 and len(g.token_bytes[V - 1]) > 1, "a drawn multi-byte token"
    assert toks[14] == E_ID and int(rstate[14]) == 6, "a drawn EOS leaves the state"
    assert int(rstate[2]) == (1 + len(g.token_bytes[V - 1])) % A
    assert sum(torch.isfinite(rv[6])) == 64 and sum(torch.isfinite(rv[4])) == 5 and sum(torch.isfinite(rv[2])) == 1


@pytest.mark.parametrize("V", SIZES)
def test_unguided_calls_are_bit_for_bit_todays(V):
    """the same logits without guide arguments, called the pre-existing way; through ops.llm; and the
    guided kernels with every row unguided (g_slot = -1): all the same bits"""
    c = _case(V)
    rows, u, B = c["rows"], c["u"], len(c["rows"])
    d_logits = c["logits"].to(DEV)
    t = lambda k, dt: torch.tensor([r[k] for r in rows], dtype=dt, device=DEV)  # noqa: E731
    args = (t("inv_t", torch.float32), t("top_p", torch.float64), t("pen", torch.float32),
            torch.tensor(u, dtype=torch.float64, device=DEV), t("greedy", torch.int32), t("seen_slot", torch.int32))
    outs = []
    for how in ("raw", "ops", "guided_off"):
        seen = c["seen"].to(DEV)
        ids, tok = torch.empty(B, dtype=torch.long, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
        v = torch.empty((B, K), dtype=torch.float32, device=DEV)
        i = torch.empty((B, K), dtype=torch.int32, device=DEV)
        lse = torch.empty(B, dtype=torch.float32, device=DEV)
        if how == "raw":
            ops.hip_ops().sample_rows(d_logits, *args, seen, t("in_id", torch.long), ids, tok, v, i, lse)
        else:
            g = None
            if how == "guided_off":
                g = _device_guide(c, rows)._replace(slot=[-1] * B)
            v, i, lse, tok, seen = lops.sample_rows(d_logits, *args, seen, t("in_id", torch.long), out_ids=ids,
                                                    guide=g)[:5]
            if g is not None:
                assert torch.equal(g.state.cpu(), torch.from_numpy(c["state0"])), "no row owns a state"
        torch.cuda.synchronize()
        outs.append((v.view(torch.int32).cpu(), i.cpu(), lse.view(torch.int32).cpu(), tok.cpu(), ids.cpu(), seen.cpu()))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)


def test_partial_guide_arguments_are_rejected():
    """the guide tensors come all together or not at all"""
    c = _case(1000)
    g = _device_guide(c, c["rows"])
    B = len(c["rows"])
    z = lambda dt: torch.zeros(B, dtype=dt, device=DEV)  # noqa: E731
    with pytest.raises(RuntimeError, match="guide tensors come together"):
        ops.hip_ops().sample_rows(c["logits"].to(DEV), z(torch.float32) + 1, z(torch.float64) + 1, z(torch.float32) + 1,
                                  z(torch.float64), z(torch.int32) + 1, z(torch.int32) - 1, c["seen"].to(DEV),
                                  z(torch.long), z(torch.long), z(torch.int32), None, None, None, g.allow, g.dfa)


# ------------------------------------------------------------------ engine
CFG = LLM_PRESETS["qwen2-0.5b"]
PATTERNS = [r"(yes|no|maybe)", r'\{"n": [0-9]{1,3}, "ok": (true|false)\}']
EOS = 299
PROMPTS = [list(np.random.default_rng(i).integers(0, 150000, 40 + 9 * i)) for i in range(7)]


def _vocab():
    multi = ["true", "false", "null", ", ", '{"', '":', '": ', '"}', "yes", "no", "maybe", "ye", "may", "be",
             '"n"', '"ok"', "10", "42", "99", "00", "07", "123", "ab", "abc", "the", " a", "tru", "e}", "€", "日本"]
    tb = [bytes([i]) for i in range(256)] + [m.encode() for m in multi]
    tb += [bytes([97 + i % 26, 97 + i // 26]) for i in range(298 - len(tb))]
    return tb + [b"", b""] + [b""] * (CFG.vocab_size - 300)


@pytest.fixture(scope="module")
def model():
    m = LLM(CFG, device="cuda")
    m.random_init(5)
    return m


def _engine(m, ingraph, max_batch=8):
    kv = PagedKVCache(CFG.num_layers, m.Hkv, CFG.head_dim, num_blocks=64, device="cuda")
    return LLMEngine(m, kv, lambda ids: m.embed_tokens(torch.tensor(ids, device="cuda")), max_batch=max_batch,
                     ingraph_sampling=ingraph)


def _gen(eng, jobs):
    rs = [eng.submit(p, len(p), SamplingParams(stop_token_ids=(EOS,), **kw)) for p, kw in jobs]
    for r in rs:
        list(r.stream(timeout=120))
    return rs


@pytest.fixture(scope="module")
def runs(model):
    """the same jobs on the host-sampling engine, then on the in-graph one (one model, computed once)"""
    vocab = _vocab()
    guides = [gd.compile_guide("regex", p, vocab, [EOS]) for p in PATTERNS]
    kinds = [{}, dict(temperature=0.9, top_p=0.95, seed=11), dict(temperature=0.8, repetition_penalty=1.3, seed=5)]
    jobs = [(PROMPTS[2 * k + w], dict(max_new_tokens=48, guide=guides[w], **kw))
            for k, kw in enumerate(kinds) for w in (0, 1)]
    jobs.append((PROMPTS[6], dict(max_new_tokens=20, temperature=0.7, seed=2)))          # the unguided request
    out = {"vocab": vocab}
    for ingraph in (False, True):
        eng = _engine(model, ingraph)
        try:
            res = {}
            for wave in ("first", "second"):
                rs = _gen(eng, jobs)
                res[wave] = [(list(r.tokens), r.finish_reason) for r in rs]
            res["stats"] = dict(eng.stats)
            _gen(eng, [(PROMPTS[0], dict(max_new_tokens=8, temperature=0.9, seed=1)),
                       (PROMPTS[1], dict(max_new_tokens=10, repetition_penalty=1.2))])
            res["after_unguided"] = dict(eng.stats)
            if ingraph:
                res["resident"] = len(eng._arena._res)
                res["free_state_rows"] = len(eng._arena._free_slots)
        finally:
            eng.close()
        out[ingraph] = res
    return out


def test_guided_graphs_equal_the_host_path(runs):
    assert [t for t, _ in runs[True]["first"]] == [t for t, _ in runs[False]["first"]]
    vocab = runs["vocab"]
    lens = set()
    for (toks, reason), which in zip(runs[True]["first"][:6], (0, 1) * 3):
        text = b"".join(vocab[t] for t in toks).decode()
        assert re.fullmatch(PATTERNS[which], text), text
        assert reason == "stop"
        lens.add(len(toks))
    assert len(lens) > 1, "the requests were to leave the batch at different steps"
    assert runs[True]["first"][6][1] == "length" and len(runs[True]["first"][6][0]) == 20
    st = runs[True]["stats"]
    assert st["guided_steps"] > 0 and st.get("lookahead_steps", 0) > 0
    assert runs[False]["stats"]["guided_steps"] == 0


def test_second_wave_reuses_slots_and_resident_guides(runs):
    assert runs[True]["second"] == runs[True]["first"], "the same seeds gave different tokens"
    assert runs[False]["second"] == runs[False]["first"]
    assert runs[True]["resident"] == 2, "each guide is uploaded once and stays resident"
    assert runs[True]["free_state_rows"] == 8, "a finished request kept its grammar-state row"


def test_unguided_batches_keep_their_mode(runs):
    before, after = runs[True]["stats"], runs[True]["after_unguided"]
    assert after.get("ingraph_sample_steps", 0) > before.get("ingraph_sample_steps", 0)
    assert after["guided_steps"] == before["guided_steps"]
