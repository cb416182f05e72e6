"""Multimodal RoPE (Qwen-VL decoders) on the GPU: the MROPE form of the RoPE + KV-write kernels
(csrc/llm.hip, per-element and tile) against the fp32 CPU reference of ops/llm.py, the
``tiny-qwen2vl`` / ``tiny-qwen3vl`` decoders against fp32 CPU models holding the same tensors, and the
engine with decode graphs and speculative decoding.

Kernel inputs are drawn as in test_qk_norm_gpu.py (randn QKV rows in bf16, shuffled slots with one
-1, gammas uniform in [0.5, 1.5]); the three position rows are drawn independently below 4000, so
every frequency that reads the wrong row shows.

Bounds (that file's): rotated q and a bf16 K cache within 0.05 absolute of the reference, which
rounds to bf16 once after the rotation; the kernels evaluate the same fp32 expression (with fused
multiply-adds, and another summation order under the norm), so a result differs by at most one bf16
step where the fp32 values straddle a rounding boundary.  Every case asserts that the reference
stays below 8 in magnitude, where one bf16 step is 2^-5 = 0.031 < 0.05.  An fp8 cache: within one
e4m3 step (0.13 relative) where the rotated bf16 value itself differs by a step, on under 2 % of the
elements.  V is copied: bit-exact."""
import numpy as np
import pytest
import torch

from lumen_amd._native import hip_ops
from lumen_amd.models.llm import LLM, LLM_PRESETS
from lumen_amd.models.vlm import VLM, VLM_PRESETS
from lumen_amd.ops import llm
from lumen_amd.runtime.engine import LLMEngine, SamplingParams
from lumen_amd.runtime.kv_cache import PagedKVCache

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-6
IMG = 259
# (sections, interleaved) per head dim: the Qwen2-VL and Qwen3-VL layouts (at 128 the released models')
LAYOUTS = {32: (((4, 6, 6), False), ((6, 5, 5), True)),
           64: (((8, 12, 12), False), ((12, 10, 10), True)),
           128: (((16, 24, 24), False), ((24, 20, 20), True))}


def _cache(NB, Hkv, D, g, fp8):
    k = torch.randn(NB, Hkv, 64, D, generator=g).bfloat16()
    v = torch.randn(NB, Hkv, D, 64, generator=g).bfloat16()
    return (k.to(torch.float8_e4m3fn), v.to(torch.float8_e4m3fn)) if fp8 else (k, v)


def _norm(D, g):
    return torch.rand(D, generator=g) + 0.5, torch.rand(D, generator=g) + 0.5, EPS


def _dev(qk):
    return (qk[0].to(DEV), qk[1].to(DEV), qk[2]) if qk is not None else None


def _pos3(T, g):
    """three distinct position rows below 4000"""
    pos = torch.randint(0, 4000, (3, T), generator=g, dtype=torch.int32)
    assert all(not torch.equal(pos[a], pos[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
    return pos


def _check(T, H, Hkv, D, fp8, norm, mrope, pos, slots, NB, seed):
    g = torch.Generator().manual_seed(seed)
    x32 = torch.randn(T, (H + 2 * Hkv) * D, generator=g)
    qkv = x32.bfloat16()
    cs = llm.rope_cos_sin(4096, D, 1e6)
    qk = _norm(D, g) if norm else None
    kc, vc = _cache(NB, Hkv, D, g, fp8)
    nq = (H + Hkv) * D
    q_ref, kc_ref, vc_ref = qkv.clone(), kc.clone(), vc.clone()
    llm.rope_kv(q_ref, pos, cs, H, Hkv, D, slots, kc_ref, vc_ref, qk_norm=qk, mrope=mrope)
    # the bounds' premises, on the reference alone
    q_32 = x32.clone()
    llm.rope_kv(q_32, pos, cs, H, Hkv, D, qk_norm=qk, mrope=mrope)
    assert (q_ref[:, :nq].float() - q_32[:, :nq]).abs().max().item() < 0.05
    assert q_ref[:, :nq].float().abs().max().item() < 8.0
    assert torch.equal(q_ref[:, nq:], qkv[:, nq:])
    # the axis map matters: with the h and w rows swapped the reference moves by far more than the bound
    q_sw = qkv.clone()
    llm.rope_kv(q_sw, pos[[0, 2, 1]], cs, H, Hkv, D, qk_norm=qk, mrope=mrope)
    assert (q_sw.float() - q_ref.float()).abs().max().item() > 0.5

    q_g, kc_g, vc_g = qkv.clone().to(DEV), kc.clone().to(DEV), vc.clone().to(DEV)
    llm.rope_kv(q_g, pos.to(DEV), cs.to(DEV), H, Hkv, D, slots.to(DEV), kc_g, vc_g, qk_norm=_dev(qk), mrope=mrope)
    dq = (q_g.cpu().float() - q_ref.float()).abs()
    dk = (kc_g.cpu().float() - kc_ref.float()).abs()
    print(f"rope_kv mrope={mrope} T={T} H={H} Hkv={Hkv} D={D} fp8={fp8} norm={norm}: max dq {dq.max().item():.4f} "
          f"max dk {dk.max().item():.4f} differing k {(dk > 0).float().mean().item():.4f}")
    assert dq.max().item() < 0.05
    assert torch.equal(q_g.cpu()[:, nq:], qkv[:, nq:])              # v columns of the rows untouched
    if fp8:
        assert (dk <= 0.13 * kc_ref.float().abs() + 1e-3).all() and (dk > 0).float().mean().item() < 0.02
        assert torch.equal(vc_g.cpu().view(torch.uint8), vc_ref.view(torch.uint8))
    else:
        assert dk.max().item() < 0.05
        assert torch.equal(vc_g.cpu(), vc_ref)
    live = slots[slots >= 0]
    written = kc_g.cpu().float()[live // 64, :, live % 64]
    assert (written - kc.float()[live // 64, :, live % 64]).abs().max().item() > 0.5


# T < 64: the per-element kernel, test_qk_norm_gpu.py's shapes (one block with idle segments, two
# blocks, 16-lane segments, more rows than a wave has segments)
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("T,H,Hkv,D", [(3, 4, 2, 64), (3, 5, 1, 128), (3, 4, 2, 32), (33, 4, 2, 64)])
def test_mrope_per_element(T, H, Hkv, D, layout, norm, fp8):
    g = torch.Generator().manual_seed(T + H + D + layout)
    pos = _pos3(T, g)
    slots = torch.randperm(2 * 64, generator=g)[:T].long()
    slots[1] = -1
    _check(T, H, Hkv, D, fp8, norm, LAYOUTS[D][layout], pos, slots, 2, seed=300 + T + H + D + layout)


# T = 70: one full 64-row tile plus a ragged tile of 6 rows, the slots running through the blocks
# from an unaligned start
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("H,Hkv,D", [(4, 2, 64), (3, 1, 128)])
def test_mrope_tiles(H, Hkv, D, layout, norm, fp8):
    T, start = 70, 37
    g = torch.Generator().manual_seed(H + D + layout)
    pos = _pos3(T, g)
    table = torch.tensor([2, 0, 1])
    p = torch.arange(start, start + T)
    slots = (table[p // 64] * 64 + p % 64).long()
    _check(T, H, Hkv, D, fp8, norm, LAYOUTS[D][layout], pos, slots, 3, seed=400 + H + D + layout)


def _inputs(T, H, Hkv, D, g):
    qkv = torch.randn(T, (H + 2 * Hkv) * D, generator=g).bfloat16()
    pos = torch.randint(0, 4000, (T,), generator=g, dtype=torch.int32)
    slots = torch.randperm(2 * 64, generator=g)[:T].long()
    slots[2] = -1
    kc, vc = _cache(2, Hkv, D, g, False)
    return qkv, pos, slots, kc, vc


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("T", [5, 70])                               # per-element and tile kernels
def test_equal_axes_are_the_plain_kernels_bit_for_bit(T, norm):
    H, Hkv = 4, 2
    for D in (64, 128):
        g = torch.Generator().manual_seed(7 + T + D)
        cs = llm.rope_cos_sin(4096, D, 1e6).to(DEV)
        qkv, pos, slots, kc, vc = _inputs(T, H, Hkv, D, g)
        qk = _dev(_norm(D, g)) if norm else None
        outs = []
        for mrope in (None, *LAYOUTS[D]):
            q, k, v = qkv.to(DEV), kc.to(DEV), vc.to(DEV)
            p = pos.to(DEV) if mrope is None else pos.to(DEV).expand(3, T).contiguous()
            llm.rope_kv(q, p, cs, H, Hkv, D, slots.to(DEV), k, v, qk_norm=qk, mrope=mrope)
            outs.append((q, k, v))
        assert not torch.equal(outs[0][0], qkv.to(DEV))
        for o in outs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))


def test_calls_without_mrope_are_unchanged():
    """mrope=None is the call without the argument, bit for bit, for the per-element and the tile
    kernel, with and without the norm, and so is the raw op called with its previous argument lists."""
    H, Hkv, D = 4, 2, 64
    g = torch.Generator().manual_seed(5)
    cs = llm.rope_cos_sin(4096, D, 1e6).to(DEV)
    qg, kg, _ = _dev(_norm(D, g))
    for T in (5, 70):
        qkv, pos, slots, kc, vc = _inputs(T, H, Hkv, D, g)
        pos, slots = pos.to(DEV), slots.to(DEV)
        for qk in (None, (qg, kg, EPS)):
            outs = []
            for mode in ("omitted", "none", "raw"):
                q, k, v = qkv.to(DEV), kc.to(DEV), vc.to(DEV)
                if mode == "omitted":
                    llm.rope_kv(q, pos, cs, H, Hkv, D, slots, k, v, qk_norm=qk)
                elif mode == "none":
                    llm.rope_kv(q, pos, cs, H, Hkv, D, slots, k, v, qk_norm=qk, mrope=None)
                elif qk is None:
                    hip_ops().rope_kv(q, pos, cs, slots, k, v, H, Hkv, D)
                else:
                    hip_ops().rope_kv(q, pos, cs, slots, k, v, H, Hkv, D, qg, kg, EPS)
                outs.append((q, k, v))
            for o in outs[1:]:
                assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))
            # and they are the reference's rotation (the parent's bound), not merely equal to each other
            q_ref = qkv.clone()
            llm.rope_kv(q_ref, pos.cpu(), cs.cpu(), H, Hkv, D,
                        qk_norm=(qg.cpu(), kg.cpu(), EPS) if qk is not None else None)
            assert (outs[0][0].cpu().float() - q_ref.float()).abs().max().item() < 0.05


def test_mrope_argument_errors():
    H, Hkv, D, T = 4, 2, 64, 2
    qkv = torch.randn(T, (H + 2 * Hkv) * D, generator=torch.Generator().manual_seed(6)).bfloat16().to(DEV)
    cs = llm.rope_cos_sin(64, D, 1e6).to(DEV)
    p1 = torch.zeros(T, dtype=torch.int32, device=DEV)
    p3 = torch.zeros(3, T, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="sum to head_dim / 2"):
        llm.rope_kv(qkv.clone(), p3, cs, H, Hkv, D, mrope=((8, 12, 13), False))
    with pytest.raises(ValueError, match="three sections"):
        llm.rope_kv(qkv.clone(), p3, cs, H, Hkv, D, mrope=((16, 16), True))
    with pytest.raises(ValueError, match=r"pos \[3, 2\]"):
        llm.rope_kv(qkv.clone(), p1, cs, H, Hkv, D, mrope=((8, 12, 12), False))
    with pytest.raises(ValueError, match="needs mrope"):
        llm.rope_kv(qkv.clone(), p3, cs, H, Hkv, D)
    # the raw op checks for itself
    axes = llm.mrope_axes(D, (8, 12, 12))
    raw = lambda pos, ax: hip_ops().rope_kv(qkv.clone(), pos, cs, None, qkv, qkv, H, Hkv, D, None, None, 0.0, ax)  # noqa: E731
    with pytest.raises(RuntimeError, match="mrope"):
        raw(p1, axes)
    with pytest.raises(RuntimeError, match="pos int32"):
        raw(p3, None)
    with pytest.raises(RuntimeError, match="mrope"):
        raw(p3, axes[:16])
    with pytest.raises(RuntimeError, match="mrope"):
        raw(p3, torch.full((D // 2,), 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="mrope"):
        raw(p3, axes.to(DEV))
    raw(p3, axes)                                                     # and accepts the well-formed call


# ------------------------------------------------------------------ models
def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.float().cpu().flatten(), b.float().cpu().flatten(), dim=0).item()


def _pair(preset, seed):
    """An fp32 CPU model and a bf16 GPU model holding the same (bf16-valued) tensors: only the kernels differ."""
    cfg = LLM_PRESETS[preset]
    cpu = LLM(cfg, dtype=torch.float32, device="cpu")
    cpu.random_init(seed)
    cpu.load_state_dict({k: v.bfloat16().float() for k, v in cpu.state_dict().items()})
    gpu = LLM(cfg, device=DEV)
    sd = gpu.state_dict()
    gpu.load_state_dict({k: v.to(sd[k].dtype) for k, v in cpu.state_dict().items()})
    return cpu, gpu


@pytest.fixture(scope="module", params=["tiny-qwen2vl", "tiny-qwen3vl"])
def pair(request):
    return _pair(request.param, 1)


class _Spy:
    """Records the GPU calls of an ops.llm function: (first positional after q, keywords)."""

    def __init__(self, monkeypatch, name):
        self.calls, fn = [], getattr(llm, name)

        def wrapped(q, *a, **kw):
            if q.is_cuda:
                self.calls.append((a, kw))
            return fn(q, *a, **kw)

        monkeypatch.setattr(llm, name, wrapped)


def _image_prompt(T, seed):
    """4 text ids, a 4 x 4 image, text up to T tokens -> (ids, pos3 [3, T], delta = -12)"""
    g = np.random.default_rng(seed)
    ids = [int(t) for t in g.integers(0, IMG, 4)] + [IMG] * 16 + [int(t) for t in g.integers(0, IMG, T - 20)]
    pos3, delta = llm.mrope_positions(ids, IMG, (4, 4))
    assert delta == -12 and pos3.shape[1] == T
    return ids, pos3, delta


@pytest.mark.parametrize("T", [40, 76])          # 76 rows take the tile kernel
def test_prefill_and_decode_match_cpu_reference(pair, T, monkeypatch):
    cpu, gpu = pair
    cfg = cpu.cfg
    ids, pos3, delta = _image_prompt(T, 11 + T)
    t = torch.tensor(ids)
    kvs = {}
    for m, dev, dt in ((cpu, "cpu", torch.float32), (gpu, DEV, torch.bfloat16)):
        kvs[dev] = kv = PagedKVCache(cfg.num_layers, m.Hkv, cfg.head_dim, num_blocks=4, device=dev, dtype=dt)
        kv.blocks.reserve(1, T + 4)
    rope = _Spy(monkeypatch, "rope_kv")
    ref = cpu.prefill(cpu.embed_tokens(t), kvs["cpu"], torch.from_numpy(kvs["cpu"].slots(1, 0, T)), pos3=pos3)
    got = gpu.prefill(gpu.embed_tokens(t.to(DEV)), kvs[DEV], torch.from_numpy(kvs[DEV].slots(1, 0, T)).to(DEV),
                      pos3=pos3.to(DEV))
    assert _cos(got, ref) > 0.99, _cos(got, ref)
    # every prefill launch is the three-axis form, fed the prompt's positions
    assert len(rope.calls) == cfg.num_layers
    for a, kw in rope.calls:
        assert kw.get("mrope") == cfg.mrope and tuple(a[0].shape) == (3, T) and torch.equal(a[0].cpu(), pos3)
    # decode steps: 1-D RoPE at cache index + delta, no launch carries mrope
    rope.calls.clear()
    dec = _Spy(monkeypatch, "paged_decode")
    tok = int(ref[0].argmax())
    for i in range(3):
        out = {}
        for m, dev in ((cpu, "cpu"), (gpu, DEV)):
            kv = kvs[dev]
            d = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)  # noqa: E731
            out[dev] = m.decode(d([tok], torch.long), d([T + i + delta], torch.int32),
                                torch.from_numpy(kv.slots(1, T + i, 1)).to(dev), kv,
                                torch.from_numpy(kv.block_table([1])).to(dev), d([T + i + 1], torch.int32))
        assert _cos(out[DEV], out["cpu"]) > 0.99, (i, _cos(out[DEV], out["cpu"]))
        tok = int(out["cpu"][0].argmax())
    assert len(dec.calls) == 3 * cfg.num_layers
    assert len(rope.calls) == (3 * cfg.num_layers if cfg.qk_norm else 0)      # without the norm the attention kernel rotates
    assert all(kw.get("mrope") is None and a[0].dim() == 1 for a, kw in rope.calls)
    for a, kw in dec.calls:
        assert (kw.get("rope") is None) == cfg.qk_norm
        if kw.get("rope") is not None:
            assert kw["rope"][0].dim() == 1 and int(kw["rope"][0][0]) - delta in range(T, T + 3)


# ------------------------------------------------------------------ engine
CFG = LLM_PRESETS["tiny-qwen3vl"]
WEIGHTS = 1
NEW = 24
# The engine tests' two prompts: 4 text ids, a 4 x 4 image (its rows are the placeholder token's
# embedding, the same values on both devices), 20 text ids, drawn by np.random.default_rng(seed)
# below the image token id.  A plain step attends through paged_decode, a verify step through
# paged_verify and a graph replay may split the context differently from an eager step, so token
# equality needs arg-maxes that are no near-ties (test_qwen3_gpu.py's method): the seeds were picked
# from the fp32 CPU reference alone (weights of seed WEIGHTS rounded to bf16 values, prefill with the
# image's positions, decode at cache index + delta) as the two of seeds 0 .. 2999 with the widest
# top-2 gap over all 24 greedy positions (0.176 and 0.142).  test_engine_prompts_reference_margin
# asserts the margin.
PAIR_SEEDS = (1406, 233)


def _engine_prompt(seed):
    p = [int(t) for t in np.random.default_rng(seed).integers(0, IMG, 24)]
    return p[:4] + [IMG] * 16 + p[4:]


PAIR = [_engine_prompt(s) for s in PAIR_SEEDS]


@pytest.fixture(scope="module")
def pair3():
    return _pair("tiny-qwen3vl", WEIGHTS)


def _greedy_logits(mod, dev, dtype, prompt, n):
    """(tokens, logits [n, V] fp32 on the CPU) of ``n`` greedy tokens of the hand-driven loop: prefill
    with the prompt's three-axis positions, then one plain decode step each at cache index + delta"""
    kv = PagedKVCache(CFG.num_layers, mod.Hkv, CFG.head_dim, num_blocks=8, device=dev, dtype=dtype)
    assert kv.blocks.reserve(1, len(prompt) + n)
    t = lambda a, dt: torch.tensor(np.asarray(a), device=dev, dtype=dt)  # noqa: E731
    P = len(prompt)
    pos3, delta = llm.mrope_positions(prompt, IMG, (4, 4))
    assert delta == -12
    lg = mod.prefill(mod.embed_tokens(t(prompt, torch.long)), kv, t(kv.slots(1, 0, P), torch.long), pos3=pos3.to(dev))
    out, toks = [lg[0].float().cpu()], []
    bt = t(kv.block_table([1]), torch.int32)
    for i in range(n):
        toks.append(int(out[-1].argmax()))
        if i < n - 1:
            lg = mod.decode(t(toks[-1:], torch.long), t([P + i + delta], torch.int32),
                            t(kv.slots(1, P + i, 1), torch.long), kv, bt, t([P + i + 1], torch.int32))
            out.append(lg[0].float().cpu())
    return toks, torch.stack(out)


def _run(m, prompts, fed=None):
    kv = PagedKVCache(CFG.num_layers, m.Hkv, CFG.head_dim, num_blocks=48, device=DEV, dtype=torch.bfloat16)
    eng = LLMEngine(m, kv, lambda ids: m.embed_tokens(torch.tensor(ids, device=DEV)), max_batch=4, use_graphs=True)
    if fed is not None:      # what the decode graphs are fed: (pos, ctx) of every plain and verify step
        launch, verify = eng.graphs.launch, eng.graphs.launch_verify
        eng.graphs.launch = lambda ids, pos, slots, bt, ctx, **kw: (
            fed.append(("step", np.array(pos), np.array(ctx))), launch(ids, pos, slots, bt, ctx, **kw))[1]
        eng.graphs.launch_verify = lambda ids, pos, slots, bt, ctx, n_rows, T, *a, **kw: (
            fed.append(("verify", np.array(pos).reshape(-1, T), np.array(ctx), np.array(n_rows))),
            verify(ids, pos, slots, bt, ctx, n_rows, T, *a, **kw))[1]
    try:
        rs = [eng.submit(p, len(p), SamplingParams(max_new_tokens=NEW), prompt_ids=p,
                         rope_pos=llm.mrope_positions(p, IMG, (4, 4))[0]) for p in prompts]
        for r in rs:
            for _ in r.stream(timeout=120):
                pass
        assert eng.graphs is not None, "the decode graphs were dropped"
        modes = sorted({k[2] for k in eng.graphs.graphs})
        return [list(r.tokens) for r in rs], dict(eng.stats), modes
    finally:
        eng.close()


def test_engine_graphs_match_the_eager_loop(pair3, monkeypatch):
    """Decode graphs on: the tokens of requests with an image are those of the hand-driven eager loop
    on the same model, and every step the graphs were fed sat at cache index + delta."""
    _, gpu = pair3
    monkeypatch.delenv("LUMEN_SPEC_DECODE", raising=False)
    want = [_greedy_logits(gpu, DEV, torch.bfloat16, p, NEW)[0] for p in PAIR]
    fed = []
    toks, st, modes = _run(gpu, PAIR, fed)
    assert toks == want
    assert st["spec_steps"] == 0 and fed and all(f[0] == "step" for f in fed)
    for _, pos, ctx in fed:
        assert np.array_equal(pos, ctx - 1 - 12), (pos, ctx)          # ctx counts the fed token: index = ctx - 1
    # a request without an image through the same engine code: delta 0, positions = cache indices
    fed = []
    text = [t if t != IMG else 7 for t in PAIR[0]]
    _run(gpu, [text], fed)
    assert all(np.array_equal(pos, ctx - 1) for _, pos, ctx in fed)


def test_engine_speculation_keeps_the_tokens(pair3, monkeypatch):
    """LUMEN_SPEC_DECODE=ngram gives the tokens of speculation off; verify rows sit at ctx + delta + i."""
    _, gpu = pair3
    monkeypatch.delenv("LUMEN_SPEC_DECODE", raising=False)
    base, st, _ = _run(gpu, PAIR)
    assert st["spec_steps"] == 0 and all(len(t) == NEW for t in base)
    monkeypatch.setenv("LUMEN_SPEC_DECODE", "ngram")
    fed = []
    toks, st, modes = _run(gpu, PAIR, fed)
    print(f"ngram: {st['spec_steps']} verify + {st['decode_steps']} plain steps, "
          f"{st['spec_accepted']}/{st['spec_drafted']} accepted, graph modes {modes}")
    assert toks == base
    assert st["spec_steps"] > 0 and "verify" in modes
    ver = [f for f in fed if f[0] == "verify"]
    assert ver
    for _, pos, ctx, n_rows in ver:
        for b in range(len(ctx)):
            n = int(n_rows[b])
            assert np.array_equal(pos[b, :n], ctx[b] - n - 12 + np.arange(n)), (pos[b], ctx[b], n)


def test_engine_prompts_reference_margin(pair3):
    """The margin the engine tests' token equality rests on (test_qwen3_gpu.py's): two GPU paths that
    each stay within err of the fp32 reference's logits pick the same token wherever the reference's
    top-2 gap exceeds 2 err; the prompts must give twice that room at every position: gap >= 4 err,
    err the largest |GPU - reference| logit error of the plain decode run."""
    cpu, gpu = pair3
    for p in PAIR:
        gt, gl = _greedy_logits(gpu, DEV, torch.bfloat16, p, NEW)
        ct, cl = _greedy_logits(cpu, "cpu", torch.float32, p, NEW)
        assert gt == ct, "the GPU run left the reference's tokens"
        top2 = cl.topk(2, dim=1).values
        gap = float((top2[:, 0] - top2[:, 1]).min())
        err = float((gl - cl).abs().max())
        print(f"reference margin: min top-2 gap {gap:.4f}, max |GPU - reference| {err:.4f}, ratio {gap / err:.1f}")
        assert gap >= 4.0 * err, (gap, err)


def test_vlm_end_to_end():
    """tiny-qwen3vl with the ViT tower through the engine: the prompt's positions come from the
    expanded ids, the image rows from the tower, and the run ends with the asked-for tokens."""
    vlm = VLM(VLM_PRESETS["tiny-qwen3vl"], device=DEV)
    vlm.random_init(2)
    vlm.eval()
    img = torch.randint(0, 256, (32, 32, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    ids = [5, 6, 7, IMG, 8, 9, 10, 11]
    full, starts = vlm.expand_image_tokens(ids, 1)
    pos3, delta = vlm.rope_positions(full)
    assert starts == [3] and delta == -12
    x = vlm.build_prefill(ids, [img.to(DEV)])
    assert tuple(x.shape) == (len(full), CFG.hidden_size) and torch.isfinite(x.float()).all()
    kv = PagedKVCache(CFG.num_layers, vlm.llm.Hkv, CFG.head_dim, num_blocks=8, device=DEV, dtype=torch.bfloat16)
    eng = LLMEngine(vlm.llm, kv, lambda a: x.clone(), max_batch=2, use_graphs=True)
    fed, launch = [], eng.graphs.launch
    eng.graphs.launch = lambda i, pos, slots, bt, ctx, **kw: (fed.append((np.array(pos), np.array(ctx))),
                                                              launch(i, pos, slots, bt, ctx, **kw))[1]
    try:
        r = eng.submit(ids, len(full), SamplingParams(max_new_tokens=8), prompt_ids=full, rope_pos=pos3)
        for _ in r.stream(timeout=120):
            pass
        assert len(r.tokens) == 8 and r.rope_delta == -12 and r.finish_reason is not None
        assert fed and all(np.array_equal(pos, ctx - 1 - 12) for pos, ctx in fed)
    finally:
        eng.close()
