"""Speculative decoding of sampled and penalised requests on the GPU: the verify form of the device
sampler (csrc/sampler.hip) against its CPU reference and against the existing HIP sample_rows run
row by row, and the engine's sampled verify step (Qwen2-0.5B, random weights) eager and as a
captured graph."""
import numpy as np
import pytest
import torch

from lumen_amd.models.llm import LLM, LLM_PRESETS
from lumen_amd.ops import llm as lops
from lumen_amd.runtime.engine import LLMEngine, SamplingParams
from lumen_amd.runtime.kv_cache import PagedKVCache
from test_sample_verify_cpu import JUNK, build_case, call_op, check_against, single_row

pytestmark = pytest.mark.gpu
DEV = "cuda"
# 1,000: one launch.  20,481: five 4096-column chunks + a one-column chunk, V % 32 = 1 (a partial
# last bitmap word), draft tokens at columns 4095 and 4096 (case C).  151,936: the Qwen2 vocabulary.
# Cases A, B: B = 3, T = 4; case C: B = 4, T = 8 (32 rows).
OP_CASES = [(1000, "A"), (1000, "B"), (1000, "C"), (20481, "A"), (20481, "C"), (151936, "C")]


@pytest.mark.parametrize("V,name", OP_CASES)
def test_op_matches_reference_and_the_row_by_row_hip_sampler(V, name):
    c = build_case(V, name)
    # the CPU reference of the whole launch is the row-by-row composition build_case holds (at the
    # Qwen2 vocabulary that is taken from the smaller sizes: the reference runs every row twice otherwise)
    if V <= 20481:
        check_against(c, call_op(c, c["logits"], c["seen"].clone()))
    d_logits = c["logits"].to(DEV)
    keep = d_logits.clone()
    out = call_op(c, d_logits, c["seen"].to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(d_logits, keep), "the logits are read only"
    check_against(c, out, lse_exact=False)
    if V > 4097 and name == "C":
        ids = set(int(t) for t in c["in_ids"])
        assert {4095, 4096} <= ids, "draft tokens either side of the first chunk edge"
    # the existing HIP sample_rows, one live row at a time with the row's penalty set as its bitmap
    v, i, lse, tok = (t.cpu() for t in out[:4])
    T = c["T"]
    for b, sq in enumerate(c["seqs"]):
        old = c["sets"].get(sq["slot"], set())
        x = [int(t) for t in c["in_ids"][b * T:b * T + sq["n"]]]
        for q in range(sq["n"]):
            r = b * T + q
            hv, hi, hlse, htok = single_row(lops.sample_rows, d_logits[r], sq, float(c["u"][r]), old | set(x[:q]), x[q], V)
            assert torch.equal(v[r].view(torch.int32), hv.view(torch.int32)) and torch.equal(i[r], hi), (b, q)
            assert np.float32(lse[r]).view(np.int32) == np.float32(hlse).view(np.int32), (b, q)
            assert int(tok[r]) == htok, (b, q)


@pytest.mark.parametrize("V,name", [(1000, "B"), (151936, "C")])
def test_tokens_without_the_candidate_outputs(V, name):
    """the verify graph's call: no candidate outputs, so greedy rows run a single merge round"""
    c = build_case(V, name)
    v, i, lse, tok, n_acc, seen = call_op(c, c["logits"].to(DEV), c["seen"].to(DEV), candidates=False)
    torch.cuda.synchronize()
    assert v is None and i is None and lse is None
    w = c["want"]
    assert torch.equal(tok.cpu(), w["tok"]) and torch.equal(n_acc.cpu(), w["n_acc"])
    assert torch.equal(seen.cpu(), w["seen"]) and torch.equal(seen.cpu()[JUNK], c["seen"][JUNK])


# ------------------------------------------------------------------ engine
CFG = LLM_PRESETS["qwen2-0.5b"]
NEW, SPEC = 24, 3
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float8_e4m3fn], ids=["bf16", "fp8"])
# Eager launches size the attention splits from the batch's real block-table width and the graphs
# from its width bucket (8 blocks here); both give two splits, and so the same bits, for tables of 5
# to 8 blocks.  The prompts of the eager-against-graphs jobs are that long: 300 + 24 tokens = 6 blocks.
LONG = [[int(t) for t in np.random.default_rng(s).integers(0, 150000, 300)] for s in (51, 52, 53, 54)]
SAMPLED = dict(temperature=0.8, top_p=0.9, seed=1)
PENALISED = dict(repetition_penalty=1.3)
JOB_REQS = {"sampled": [(LONG[0], SAMPLED)], "penalised": [(LONG[0], PENALISED)],
            "mixed": [(LONG[0], {}), (LONG[1], SAMPLED), (LONG[2], PENALISED), (LONG[3], dict(SAMPLED, **PENALISED))]}
# The prompt of the test that asserts equality with speculation off.  A verify step rounds
# differently from a decode step (test_spec_decode_gpu.py), so equality needs a margin, and the
# prompt was picked from the fp32 CPU reference alone, by the scan that chose
# test_spec_decode_gpu.PAIR (24-token prompts of default_rng(seed), 24 greedy tokens on the
# PAIR_WEIGHTS model, the smallest top-2 gap over the 24 positions), run on the penalised logits.
# A random model repeats its dominant token, and the penalty pulls exactly that token's logit
# towards the runner-up: at penalty 1.3 none of the 7,400 seeds scanned (0 .. 5950, 6000 .. 7550)
# keeps a gap of 0.55 (the two PAIR seeds fall to 0.139 and 0.015).  At penalty 1.1 seed 364 keeps
# 0.660 (0.998 unpenalised; seed 2026: 0.496), so the request is seed 364 at penalty 1.1.
# test_penalised_reference_margin asserts the margin.
PAIR_WEIGHTS = 8
PEN = 1.1
PEN_SEED = 364
PEN_PROMPT = [int(t) for t in np.random.default_rng(PEN_SEED).integers(0, 150000, 24)]


@pytest.fixture(scope="module")
def model():
    m = LLM(CFG, device=DEV)
    m.random_init(8)
    return m


class Script:
    """A drafter that replays given token sequences by position: ``kind`` oracle proposes them as
    they are, half a right first and a wrong second token; unknown prompts get no draft."""

    def __init__(self, kind, truths):
        self.kind, self.truths = kind, truths          # [(prompt, tokens)]

    def __call__(self, token_ids, k):
        for p, truth in self.truths:
            if list(token_ids[:len(p)]) == p:
                n = len(token_ids) - len(p)
                t = list(truth[n:n + k])
                if self.kind == "half":
                    t = t[:1] + [(x + 1) % 150000 for x in t[1:2]]
                return t
        return []


def _run(m, dtype, graphs, reqs, drafter=None, spec_sampling=True):
    """reqs [(prompt, SamplingParams kwargs)], all joining the batch in the same engine iteration
    (admission is held until every request is queued, so the batch's history does not depend on
    thread timing) -> ([tokens], stats, captured graph modes)"""
    kv = PagedKVCache(CFG.num_layers, m.Hkv, CFG.head_dim, num_blocks=48, device=DEV, dtype=dtype)
    eng = LLMEngine(m, kv, lambda ids: m.embed_tokens(torch.tensor(ids, device=DEV)), max_batch=4,
                    use_graphs=graphs, drafter=drafter, spec_tokens=SPEC, spec_sampling=spec_sampling)
    try:
        hold, eng.max_prefill = eng.max_prefill, 0
        rs = [eng.submit(p, len(p), SamplingParams(max_new_tokens=NEW, **sp), prompt_ids=p) for p, sp in reqs]
        eng.max_prefill = hold
        for r in rs:
            for _ in r.stream(timeout=120):
                pass
        modes = sorted({k[2] for k in eng.graphs.graphs}) if eng.graphs is not None else []
        assert graphs == (eng.graphs is not None), "the graphs were dropped"
        if eng._slots is not None:
            assert sorted(eng._slots._free_slots) == list(range(4)), "a bitmap slot was not given back"
        return [list(r.tokens) for r in rs], dict(eng.stats), modes
    finally:
        eng.close()


def _agree(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


@pytest.mark.parametrize("job", ["sampled", "penalised", "mixed"])
@DTYPES
def test_engine_graphs_and_eager_give_the_same_tokens(model, dtype, job):
    """A random model's 64 candidates lie within the bf16 rounding of the logits, and a verify step
    rounds differently from a decode step, so a sampled request leaves its run with speculation off
    early (printed, not asserted).  The oracle therefore replays a run made of verify steps: one
    under a drafter whose fixed proposal is (as good as) never drawn."""
    reqs = JOB_REQS[job]
    base, st, _ = _run(model, dtype, False, reqs, spec_sampling=False)
    assert st["spec_steps"] == 0 and all(len(t) == NEW for t in base)
    first, st, _ = _run(model, dtype, False, reqs, lambda ids, k: [11, 12, 13][:k])
    assert st["spec_sample_steps"] > 0 and all(len(t) == NEW for t in first)
    for a, b in zip(base, first):       # not asserted: verify steps and decode steps round differently
        print(f"{job} {dtype}: agrees with speculation off for {_agree(a, b)} of {NEW} tokens")
    script = Script("oracle", [(p, t) for (p, _), t in zip(reqs, first)])
    eager, st_e, _ = _run(model, dtype, False, reqs, script)
    graph, st_g, modes = _run(model, dtype, True, reqs, script)
    print(f"{job} {dtype}: graphs {st_g['spec_sample_steps']} sampled verify + {st_g['decode_steps']} plain steps, "
          f"{st_g['spec_accepted']}/{st_g['spec_drafted']} accepted")
    assert graph == eager
    assert "verify_sample" in modes, "no verify_sample graph was captured"
    for st in (st_e, st_g):
        assert st["spec_sample_steps"] > 0 and st["spec_accepted"] > 0
    assert all(len(t) == NEW for t in graph)


@pytest.fixture(scope="module")
def pair_models():
    """(GPU model, fp32 CPU reference) with the same bf16-valued weights, as in test_spec_decode_gpu.py"""
    ref = LLM(CFG, dtype=torch.float32, device="cpu")
    ref.random_init(PAIR_WEIGHTS)
    ref.load_state_dict({k: v.bfloat16().float() for k, v in ref.state_dict().items()})
    m = LLM(CFG, device=DEV)
    m.load_state_dict({k: v.bfloat16() for k, v in ref.state_dict().items()})
    return m, ref


@DTYPES
def test_penalised_greedy_request_equals_speculation_off(pair_models, dtype):
    """one penalised greedy request on the margin prompt: the tokens of speculation off, under a drafter
    that is always right and one that is right once per step (test_penalised_reference_margin holds
    the margin this rests on)"""
    m = pair_models[0]
    reqs = [(PEN_PROMPT, dict(repetition_penalty=PEN))]
    base, st, _ = _run(m, dtype, True, reqs, spec_sampling=False)
    assert st["spec_steps"] == 0 and len(base[0]) == NEW
    for kind in ("oracle", "half"):
        toks, st, modes = _run(m, dtype, True, reqs, Script(kind, [(PEN_PROMPT, base[0])]))
        assert toks == base, kind
        assert st["spec_sample_steps"] > 0 and st["spec_accepted"] > 0 and "verify_sample" in modes


def _penalised_logits(mod, dev, dtype, prompt, n, pen):
    """(tokens, penalised logits [n, V] fp32 on the CPU) of ``n`` greedy tokens under a repetition
    penalty over the generated tokens, one plain decode step each"""
    kv = PagedKVCache(CFG.num_layers, mod.Hkv, CFG.head_dim, num_blocks=8, device=dev, dtype=dtype)
    assert kv.blocks.reserve(1, len(prompt) + n)
    t = lambda a, dt: torch.tensor(np.asarray(a), device=dev, dtype=dt)  # noqa: E731
    P = len(prompt)
    lg = mod.prefill(mod.embed_tokens(t(prompt, torch.long)), kv, t(kv.slots(1, 0, P), torch.long))
    out, toks = [], []
    bt = t(kv.block_table([1]), torch.int32)
    for i in range(n):
        x = lg[0].float().cpu().clone()
        if toks:
            lops.rep_penalty_(x[None], [toks], [pen])
        out.append(x)
        toks.append(int(x.argmax()))
        if i < n - 1:
            lg = mod.decode(t(toks[-1:], torch.long), t([P + i], torch.int32), t(kv.slots(1, P + i, 1), torch.long),
                            kv, bt, t([P + i + 1], torch.int32))
    return toks, torch.stack(out)


def test_penalised_reference_margin(pair_models):
    """The margin the equality above rests on: at every position of the non-speculative penalised
    run of PEN_PROMPT the fp32 CPU reference's top-2 gap of the penalised logits is at least 10x the
    largest |GPU - reference| error of the penalised logits (bf16 model, bf16 cache)."""
    model, ref = pair_models
    gt, gl = _penalised_logits(model, DEV, torch.bfloat16, PEN_PROMPT, NEW, PEN)
    ct, cl = _penalised_logits(ref, "cpu", torch.float32, PEN_PROMPT, NEW, PEN)
    assert gt == ct, "the GPU run left the reference's tokens"
    top2 = cl.topk(2, dim=1).values
    gap = float((top2[:, 0] - top2[:, 1]).min())
    err = float((gl - cl).abs().max())
    print(f"penalised reference margin: min top-2 gap {gap:.4f}, max |GPU - reference| {err:.4f}, ratio {gap / err:.1f}")
    assert gap >= 10.0 * err, (gap, err)
