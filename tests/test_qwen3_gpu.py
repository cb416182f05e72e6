"""The Qwen3 decoder (per-head q / k RMSNorm before RoPE) on the GPU: ``tiny-qwen3`` (head_dim 64,
heads x head_dim != hidden) in bf16 against the fp32 CPU model holding the same tensors -- prefill
(per-element and tile RoPE kernels), decode, verify, decode-graph replay and the engine with
speculative decoding."""
import numpy as np
import pytest
import torch

from lumen_amd import ops
from lumen_amd.models.llm import LLM, LLM_PRESETS
from lumen_amd.ops import llm as lops
from lumen_amd.runtime.engine import LLMEngine, SamplingParams
from lumen_amd.runtime.kv_cache import PagedKVCache

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = LLM_PRESETS["tiny-qwen3"]
WEIGHTS = 1
NEW = 24
# The engine test's two prompts.  A plain step attends through paged_decode, a verify step through
# paged_verify, which sum in different orders, so token equality needs arg-maxes that
# are no near-ties (test_spec_decode_gpu.py's method): the seeds were picked from the fp32 CPU
# reference alone (weights of seed WEIGHTS rounded to bf16 values) as the two of the 24-token prompts
# of seeds 0 .. 2999 with the widest top-2 gap over all 24 greedy positions (0.140 and 0.122).
# test_engine_prompts_reference_margin asserts the margin.
PAIR_SEEDS = (1125, 1047)
PAIR = [[int(t) for t in np.random.default_rng(s).integers(0, CFG.vocab_size, 24)] for s in PAIR_SEEDS]


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.float().cpu().flatten(), b.float().cpu().flatten(), dim=0).item()


@pytest.fixture(scope="module")
def pair():
    """An fp32 CPU model and a bf16 GPU model holding the same (bf16-valued) tensors, the q / k norm
    weights (drawn around 1, fp32 on both) included: only the kernels differ."""
    cpu = LLM(CFG, dtype=torch.float32, device="cpu")
    cpu.random_init(WEIGHTS)
    cpu.load_state_dict({k: v.bfloat16().float() for k, v in cpu.state_dict().items()})
    gpu = LLM(CFG, device=DEV)
    sd = gpu.state_dict()
    gpu.load_state_dict({k: v.to(sd[k].dtype) for k, v in cpu.state_dict().items()})
    for lc, lg in zip(cpu.layers, gpu.layers):
        assert lg.q_norm.dtype == torch.float32 and torch.equal(lg.q_norm.cpu(), lc.q_norm)
        assert torch.equal(lg.k_norm.cpu(), lc.k_norm) and not torch.equal(lc.q_norm, lc.k_norm)
        assert (lc.q_norm - 1).abs().max() > 0.05
    assert CFG.num_heads * CFG.head_dim != CFG.hidden_size
    return cpu, gpu


class _Spy:
    """Records the GPU calls of an ops.llm function (the CPU model goes through the same functions)."""

    def __init__(self, monkeypatch, name):
        self.calls, fn = [], getattr(lops, name)

        def wrapped(q, *a, **kw):
            if q.is_cuda:
                self.calls.append(kw)
            return fn(q, *a, **kw)

        monkeypatch.setattr(lops, name, wrapped)


@pytest.mark.parametrize("T", [40, 70])          # 70 rows take the tile kernel
def test_prefill_matches_cpu_reference(pair, T, monkeypatch):
    cpu, gpu = pair
    rope = _Spy(monkeypatch, "rope_kv")
    ids = torch.randint(0, CFG.vocab_size, (T,), generator=torch.Generator().manual_seed(11))
    ref = cpu.prefill(cpu.embed_tokens(ids))
    got = gpu.prefill(gpu.embed_tokens(ids.to(DEV)))
    assert _cos(got, ref) > 0.99, _cos(got, ref)
    assert len(rope.calls) == CFG.num_layers and all(c.get("qk_norm") is not None for c in rope.calls)


def _prefilled(m, dev, B, T0):
    """B sequences of T0 + 3 b prompt tokens prefilled into a fresh paged cache."""
    kv = PagedKVCache(CFG.num_layers, m.Hkv, CFG.head_dim, num_blocks=16, device=dev,
                      dtype=torch.float32 if dev == "cpu" else torch.bfloat16)
    lens = [T0 + 3 * b for b in range(B)]
    for b, T in enumerate(lens):
        ids = torch.randint(0, CFG.vocab_size, (T,), generator=torch.Generator().manual_seed(20 + b))
        kv.blocks.reserve(b + 1, T + 8)
        m.prefill(m.embed_tokens(ids.to(dev)), kv, torch.from_numpy(kv.slots(b + 1, 0, T)).to(dev))
    return kv, lens


def _step_args(kv, lens, step, ids, dev):
    B = len(lens)
    pos = torch.tensor([T + step for T in lens], dtype=torch.int32, device=dev)
    slots = torch.cat([torch.from_numpy(kv.slots(b + 1, lens[b] + step, 1)) for b in range(B)]).to(dev)
    bt = torch.from_numpy(kv.block_table([b + 1 for b in range(B)])).to(dev)
    return ids.to(dev), pos, slots, kv, bt, pos + 1


@pytest.mark.parametrize("B", [1, 5])
def test_decode_matches_cpu_reference(pair, B, monkeypatch):
    """8 teacher-forced decode steps through a paged KV cache.  The norm sits before the rotation,
    so every GPU step of every layer goes through rope_kv with the layer's norms (the per-element
    kernel) and the attention kernel gets rotated rows: no fused RoPE that would skip the norm."""
    cpu, gpu = pair
    steps = torch.randint(0, CFG.vocab_size, (8, B), generator=torch.Generator().manual_seed(30 + B))
    kc, lens = _prefilled(cpu, "cpu", B, 40)
    kg, _ = _prefilled(gpu, DEV, B, 40)
    dec, rope = _Spy(monkeypatch, "paged_decode"), _Spy(monkeypatch, "rope_kv")
    for s in range(8):
        ref = cpu.decode(*_step_args(kc, lens, s, steps[s], "cpu"))
        got = gpu.decode(*_step_args(kg, lens, s, steps[s], DEV))
        for b in range(B):
            assert _cos(got[b], ref[b]) > 0.99, (s, b, _cos(got[b], ref[b]))
    assert len(dec.calls) == len(rope.calls) == 8 * CFG.num_layers
    assert all(c.get("qk_norm") is not None for c in rope.calls)
    assert all(c.get("rope") is None for c in dec.calls)


def test_verify_matches_cpu_decode(pair):
    """LLM.verify with T = 4 (rope_kv's per-element kernel with the norms + paged_verify) against the
    CPU model's decode logits at the same positions."""
    cpu, gpu = pair
    T = 4
    fed = torch.randint(0, CFG.vocab_size, (T,), generator=torch.Generator().manual_seed(43))
    kc, lens = _prefilled(cpu, "cpu", 1, 40)
    kg, _ = _prefilled(gpu, DEV, 1, 40)
    P = lens[0]
    ver = gpu.verify(fed.to(DEV), torch.arange(P, P + T, dtype=torch.int32, device=DEV),
                     torch.from_numpy(kg.slots(1, P, T)).to(DEV), kg, torch.from_numpy(kg.block_table([1])).to(DEV),
                     torch.tensor([P + T], dtype=torch.int32, device=DEV),
                     torch.tensor([T], dtype=torch.int32, device=DEV), T)
    assert ver.shape == (T, gpu.Vl)
    for i in range(T):
        ref = cpu.decode(*_step_args(kc, lens, i, fed[i:i + 1], "cpu"))
        assert _cos(ver[i], ref[0]) > 0.99, (i, _cos(ver[i], ref[0]))


def test_decode_graph_replay_is_bit_identical(pair):
    _, gpu = pair
    kv, lens = _prefilled(gpu, DEV, 1, 40)
    args = _step_args(kv, lens, 0, torch.tensor([7]), DEV)
    eager = gpu.decode(*args).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gpu.decode(*args)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with ops.CAPTURE_LOCK, torch.cuda.graph(graph):
        cap = gpu.decode(*args)
    outs = []
    for _ in range(2):
        cap.zero_()
        graph.replay()
        torch.cuda.synchronize()
        outs.append(cap.clone())
    assert torch.equal(outs[0], outs[1])
    assert _cos(outs[0], eager) > 0.9999


def _run(m, reqs):
    kv = PagedKVCache(CFG.num_layers, m.Hkv, CFG.head_dim, num_blocks=48, device=DEV, dtype=torch.bfloat16)
    eng = LLMEngine(m, kv, lambda ids: m.embed_tokens(torch.tensor(ids, device=DEV)), max_batch=4, use_graphs=True)
    try:
        rs = [eng.submit(p, len(p), SamplingParams(max_new_tokens=n), prompt_ids=p) for p, n in reqs]
        for r in rs:
            for _ in r.stream(timeout=120):
                pass
        modes = sorted({k[2] for k in eng.graphs.graphs})
        return [list(r.tokens) for r in rs], dict(eng.stats), modes
    finally:
        eng.close()


def test_engine_speculation_keeps_the_tokens(pair, monkeypatch):
    """Decode graphs on, two greedy requests: LUMEN_SPEC_DECODE=ngram gives the tokens of speculation off."""
    _, gpu = pair
    monkeypatch.delenv("LUMEN_SPEC_DECODE", raising=False)
    base, st, _ = _run(gpu, [(p, NEW) for p in PAIR])
    assert st["spec_steps"] == 0 and all(len(t) == NEW for t in base)
    monkeypatch.setenv("LUMEN_SPEC_DECODE", "ngram")
    toks, st, modes = _run(gpu, [(p, NEW) for p in PAIR])
    print(f"ngram: {st['spec_steps']} verify + {st['decode_steps']} plain steps, "
          f"{st['spec_accepted']}/{st['spec_drafted']} accepted, graph modes {modes}")
    assert toks == base
    assert st["spec_steps"] > 0 and "verify" in modes


def _greedy_logits(mod, dev, dtype, prompt, n):
    """(tokens, logits [n, V] fp32 on the CPU) of ``n`` greedy tokens, one plain decode step each"""
    kv = PagedKVCache(CFG.num_layers, mod.Hkv, CFG.head_dim, num_blocks=8, device=dev, dtype=dtype)
    assert kv.blocks.reserve(1, len(prompt) + n)
    t = lambda a, dt: torch.tensor(np.asarray(a), device=dev, dtype=dt)  # noqa: E731
    P = len(prompt)
    lg = mod.prefill(mod.embed_tokens(t(prompt, torch.long)), kv, t(kv.slots(1, 0, P), torch.long))
    out, toks = [lg[0].float().cpu()], []
    bt = t(kv.block_table([1]), torch.int32)
    for i in range(n):
        toks.append(int(out[-1].argmax()))
        if i < n - 1:
            lg = mod.decode(t(toks[-1:], torch.long), t([P + i], torch.int32), t(kv.slots(1, P + i, 1), torch.long),
                            kv, bt, t([P + i + 1], torch.int32))
            out.append(lg[0].float().cpu())
    return toks, torch.stack(out)


def test_engine_prompts_reference_margin(pair):
    """The margin the engine test's token equality rests on.  Two GPU paths that each stay within
    err of the fp32 reference's logits pick the same token wherever the reference's top-2 gap
    exceeds 2 err; the prompts must give twice that room at every position: gap >= 4 err, err the
    largest |GPU - reference| logit error of the plain decode run."""
    cpu, gpu = pair
    for p in PAIR:
        gt, gl = _greedy_logits(gpu, DEV, torch.bfloat16, p, NEW)
        ct, cl = _greedy_logits(cpu, "cpu", torch.float32, p, NEW)
        assert gt == ct, "the GPU run left the reference's tokens"
        top2 = cl.topk(2, dim=1).values
        gap = float((top2[:, 0] - top2[:, 1]).min())
        err = float((gl - cl).abs().max())
        print(f"reference margin: min top-2 gap {gap:.4f}, max |GPU - reference| {err:.4f}, ratio {gap / err:.1f}")
        assert gap >= 4.0 * err, (gap, err)
