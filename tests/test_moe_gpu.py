"""The sparse mixture-of-experts MLP (csrc/moe.hip) on the GPU: routing against the fp32 reference
logits within the derivable summation-order bound, the grouped expert GEMMs and the whole MLP on the
GPU's own ids against the fp32 reference on those ids, bad ids and shapes, determinism and graph
replay, then the ``tiny-qwen3-moe`` decoder (prefill, decode, verify, decode graphs, the engine)
against the fp32 CPU model holding the same tensors."""
import json
from pathlib import Path

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
CFG = LLM_PRESETS["tiny-qwen3-moe"]


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-6)).item()


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.float().cpu().flatten(), b.float().cpu().flatten(), dim=0).item()


# (T, E, k, H, I), what it exercises
SHAPES = {
    "one-token": (1, 8, 2, 128, 64),
    "mostly-empty": (5, 128, 8, 256, 128),
    "two-blocks": (37, 4, 2, 128, 64),
    "one-expert": (37, 4, 2, 128, 64),           # every token's first choice is expert 3: 37 rows, 3 blocks, ragged
    "k-equals-E": (70, 8, 8, 128, 64),
    "prefill-tile": (300, 8, 2, 128, 64),
    "layer-width": (4, 16, 8, 2048, 768),
}
_CASES = {}


def _case(name):
    """bf16 tensors of a shape on the device (generated there), their fp32 CPU copies, and -- computed
    once and shared -- the GPU's routing and the fp32 reference of the MLP on the GPU's own ids."""
    if name in _CASES:
        return _CASES[name]
    T, E, k, H, I = SHAPES[name]
    g = torch.Generator(device=DEV).manual_seed(100 + list(SHAPES).index(name))

    def rnd(*shape, std=1.0):
        return (torch.randn(shape, generator=g, device=DEV, dtype=torch.float32) * std).bfloat16()

    x = rnd(T, H)
    gate_w = rnd(E, H, std=3.0 * H ** -0.5)               # logits of std ~3: weights far from uniform
    if name == "one-expert":
        x[:, 0] = x[:, 0].abs() + 1.0
        gate_w[:, 0] = 0.0
        gate_w[3] = 0.0
        gate_w[3, 0] = 16.0                               # logit 3 >= 16, the others ~N(0, 9)
    gu_w = rnd(E, 2 * I, H, std=H ** -0.5)
    down_w = rnd(E, H, I, std=I ** -0.5)
    c = dict(T=T, E=E, k=k, H=H, I=I, x=x, gate_w=gate_w, gu_w=gu_w, down_w=down_w)
    c["cpu"] = {n: c[n].float().cpu() for n in ("x", "gate_w", "gu_w", "down_w")}
    ids, w = lops.moe_route(x, gate_w, k)
    c["ids"], c["w"] = ids, w
    c["ref"] = lops.moe_experts(c["cpu"]["x"], ids.cpu(), w.cpu(), c["cpu"]["gu_w"], c["cpu"]["down_w"])
    _CASES[name] = c
    return c


def _check_route(c, ids, w, norm_topk):
    """ids / w of the GPU against the fp32 reference logits L: every row, no exceptions."""
    T, E, k, H = c["T"], c["E"], c["k"], c["H"]
    xc, gc = c["cpu"]["x"], c["cpu"]["gate_w"]
    L = xc @ gc.t()
    # products of bf16 values are exact in fp32; the two sums differ only in their order:
    # |L_gpu - L_ref| <= 2 H 2^-24 sum_i |x_i g_i|, taken at the worst expert of the row
    delta = 2.0 * H * 2.0 ** -24 * (xc.abs() @ gc.abs().t()).max(dim=1).values
    ids, w = ids.cpu().long(), w.cpu()
    assert ids.shape == (T, k) and w.shape == (T, k)
    assert int(ids.min()) >= 0 and int(ids.max()) < E
    assert all(len(set(r)) == k for r in ids.tolist()), "ids within a row must be distinct"
    kth = torch.sort(L, dim=1, descending=True).values[:, k - 1]
    sel = torch.zeros(T, E, dtype=torch.bool).scatter_(1, ids, True)
    lo = (L - (kth - delta)[:, None])[sel]
    hi = (L - (kth + delta)[:, None])[~sel]
    print(f"route: max delta {float(delta.max()):.3e}, selected slack {float(lo.min()):.3e}, "
          f"unselected slack {float(-hi.max()) if hi.numel() else float('inf'):.3e}")
    assert (lo >= 0).all(), "a selected expert lies below the k-th reference logit by more than delta"
    assert (hi <= 0).all(), "an unselected expert lies above the k-th reference logit by more than delta"
    ref_w = lops.route_weights(L, ids, norm_topk)
    err = ((w - ref_w).abs() / ref_w.abs()).max(dim=1).values
    tol = 4.0 * delta + 1e-6
    print(f"route weights: max relative error {float(err.max()):.3e}, smallest tolerance {float(tol.min()):.3e}")
    assert (err <= tol).all(), (err / tol).max()


@pytest.mark.parametrize("name", list(SHAPES))
def test_route_against_reference_logits(name):
    c = _case(name)
    _check_route(c, c["ids"], c["w"], True)
    if name == "one-expert":
        assert (c["ids"][:, 0] == 3).all()


@pytest.mark.parametrize("name", list(SHAPES))
def test_mlp_and_experts_against_reference_on_gpu_ids(name):
    c = _case(name)
    k, E = c["k"], c["E"]
    ref, cpu = c["ref"], c["cpu"]
    got_e = lops.moe_experts(c["x"], c["ids"], c["w"], c["gu_w"], c["down_w"])
    got_m = lops.moe_mlp(c["x"], c["gate_w"], c["gu_w"], c["down_w"], k)
    torch.cuda.synchronize()
    print(f"{name}: rel experts {_rel(got_e, ref):.3e}, mlp {_rel(got_m, ref):.3e}")
    assert got_e.dtype == torch.bfloat16 and got_e.shape == ref.shape
    assert _rel(got_e, ref) < 1e-2
    assert _rel(got_m, ref) < 1e-2
    assert torch.equal(got_e, got_m), "moe_mlp is moe_route + moe_experts"
    # the check can tell: flat weights, or ids rotated by one expert, move the reference by far more
    ids_c, w_c = c["ids"].cpu(), c["w"].cpu()
    flat = lops.moe_experts(cpu["x"], ids_c, torch.full_like(w_c, 1.0 / k), cpu["gu_w"], cpu["down_w"])
    rot = lops.moe_experts(cpu["x"], (ids_c + 1) % E, w_c, cpu["gu_w"], cpu["down_w"])
    print(f"{name}: reference moves by {_rel(flat, ref):.3f} (w = 1 / k), {_rel(rot, ref):.3f} (ids + 1)")
    assert _rel(flat, ref) > 5e-2 and _rel(rot, ref) > 5e-2


def test_norm_topk_false():
    c = _case("mostly-empty")
    ids, w = lops.moe_route(c["x"], c["gate_w"], c["k"], norm_topk=False)
    _check_route(c, ids, w, False)
    assert (w.sum(1) < 0.9999).all(), "un-renormalised weights do not sum to 1"
    cpu = c["cpu"]
    ref = lops.moe_experts(cpu["x"], ids.cpu(), w.cpu(), cpu["gu_w"], cpu["down_w"])
    got = lops.moe_mlp(c["x"], c["gate_w"], c["gu_w"], c["down_w"], c["k"], norm_topk=False)
    assert _rel(got, ref) < 1e-2
    assert _rel(c["ref"], ref) > 5e-2, "the renormalised result is a different one"


def test_residual_aliasing_out():
    c = _case("two-blocks")
    cpu = c["cpu"]
    res = (torch.randn(c["T"], c["H"], generator=torch.Generator().manual_seed(7)) * 0.3).bfloat16()
    ref = lops.moe_experts(cpu["x"], c["ids"].cpu(), c["w"].cpu(), cpu["gu_w"], cpu["down_w"], residual=res.float())
    buf = res.to(DEV).clone()
    out = lops.moe_mlp(c["x"], c["gate_w"], c["gu_w"], c["down_w"], c["k"], residual=buf, out=buf)
    assert out.data_ptr() == buf.data_ptr()
    sep = lops.moe_mlp(c["x"], c["gate_w"], c["gu_w"], c["down_w"], c["k"], residual=res.to(DEV))
    assert torch.equal(buf, sep), "in place and out of place agree bit for bit"
    assert _rel(buf, ref) < 1e-2
    assert _rel(c["ref"], ref) > 5e-2, "the residual is a visible part of the result"


def test_bad_ids_contribute_nothing():
    c = _case("two-blocks")
    cpu, E = c["cpu"], c["E"]
    bad = c["ids"].clone()
    bad[0, 0], bad[5, 1], bad[36, 0] = -1, E, E + 1000
    ref = lops.moe_experts(cpu["x"], bad.cpu(), c["w"].cpu(), cpu["gu_w"], cpu["down_w"])     # skips those pairs
    got = lops.moe_experts(c["x"], bad, c["w"], c["gu_w"], c["down_w"])
    torch.cuda.synchronize()
    assert _rel(got, ref) < 1e-2
    assert _rel(got[[0, 5, 36]], ref[[0, 5, 36]]) < 1e-2
    assert _rel(c["ref"][[0, 5, 36]], ref[[0, 5, 36]]) > 5e-2, "the dropped pairs mattered"
    rest = [t for t in range(c["T"]) if t not in (0, 5, 36)]
    good = lops.moe_experts(c["x"], c["ids"], c["w"], c["gu_w"], c["down_w"])
    assert torch.equal(got[rest], good[rest]), "the other rows are untouched, bit for bit"


@pytest.mark.parametrize("H,I", [(128, 72), (48, 64)])
def test_bad_shapes_raise_before_any_launch(H, I):
    E, k, T = 4, 2, 3
    z = lambda *s: torch.zeros(s, device=DEV, dtype=torch.bfloat16)  # noqa: E731
    with pytest.raises(ValueError):
        lops.moe_mlp(z(T, H), z(E, H), z(E, 2 * I, H), z(E, H, I), k)
    with pytest.raises(ValueError):
        lops.moe_experts(z(T, H), torch.zeros(T, k, device=DEV, dtype=torch.int32),
                         torch.zeros(T, k, device=DEV), z(E, 2 * I, H), z(E, H, I))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["mostly-empty", "prefill-tile"])
def test_two_eager_runs_are_bit_identical(name):
    c = _case(name)
    a = lops.moe_mlp(c["x"], c["gate_w"], c["gu_w"], c["down_w"], c["k"])
    b = lops.moe_mlp(c["x"], c["gate_w"], c["gu_w"], c["down_w"], c["k"])
    assert torch.equal(a, b)


def test_graph_replay_follows_new_routing():
    """One captured graph serves any routing: overwrite the static input with rows that route
    differently, replay, and get the bits of an eager call on those rows."""
    c = _case("mostly-empty")
    k = c["k"]
    x2 = c["x"].flip(1).contiguous()                      # same values, other directions: other experts
    ids2, _ = lops.moe_route(x2, c["gate_w"], k)
    assert not torch.equal(ids2, c["ids"]), "the second input must route differently"
    eager1 = lops.moe_mlp(c["x"], c["gate_w"], c["gu_w"], c["down_w"], k)
    eager2 = lops.moe_mlp(x2, c["gate_w"], c["gu_w"], c["down_w"], k)
    static_x = c["x"].clone()
    side = ops.private_stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lops.moe_mlp(static_x, c["gate_w"], c["gu_w"], c["down_w"], k)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.CAPTURE_LOCK, torch.cuda.graph(graph, stream=side):
        cap = lops.moe_mlp(static_x, c["gate_w"], c["gu_w"], c["down_w"], k)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, eager1)
    static_x.copy_(x2)
    cap.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, eager2)
    assert not torch.equal(eager1, eager2)


# ------------------------------------------------------------------------------------------ the decoder
WEIGHTS = 1
GOLDEN = Path(__file__).resolve().parent / "golden" / "moe_router_margin_tokens.json"
GAP = 0.25          # the reference's k-th / (k+1)-th router-logit gap every chosen token keeps, all layers


class _RouterSpy:
    """Router logits (fp32, on the CPU, from the rows the model handed to moe_mlp) of every sparse MLP call."""

    def __init__(self):
        self.calls, self._layers, self._rows = 0, [], []
        self._fn = lops.moe_mlp

    @property
    def logits(self):
        """one [rows, E] tensor per layer, rows in call order (however the calls grouped them)"""
        return [torch.cat(r) for r in self._rows]

    def __enter__(self):
        def wrapped(h, router_w, *a, **kw):
            if router_w.data_ptr() not in self._layers:
                self._layers.append(router_w.data_ptr())
                self._rows.append([])
            self._rows[self._layers.index(router_w.data_ptr())].append(h.float().cpu() @ router_w.float().cpu().t())
            self.calls += 1
            return self._fn(h, router_w, *a, **kw)

        lops.moe_mlp = wrapped
        return self

    def __exit__(self, *exc):
        lops.moe_mlp = self._fn

    def min_gap(self, k):
        s = torch.sort(torch.cat(self.logits), dim=1, descending=True).values
        return float((s[:, k - 1] - s[:, k]).min())


def _margin(ref_spy, gpu_spy, what):
    """A near-tie at the k-th router logit would let the two models pick different experts.  The
    token sequences were built from the fp32 reference alone so that its smallest k-th / (k+1)-th gap
    over all layers and rows is wide; assert it is at least 4x the largest router-logit error of
    this run (two paths within err of the reference agree wherever the gap exceeds 2 err)."""
    assert len(ref_spy.logits) == len(gpu_spy.logits) == CFG.num_layers
    assert all(a.shape == b.shape for a, b in zip(ref_spy.logits, gpu_spy.logits))
    gap = ref_spy.min_gap(CFG.num_experts_per_tok)
    err = max(float((a - b).abs().max()) for a, b in zip(ref_spy.logits, gpu_spy.logits))
    print(f"{what}: min router gap {gap:.4f}, max |GPU - reference| router logit {err:.4f}, ratio {gap / err:.1f}")
    assert gap >= 4.0 * err, (gap, err)


def _build_tokens(cpu, n, seed):
    """How the sequences of GOLDEN were made (``python -m tests.test_moe_gpu`` from the repository root rebuilds the file; CPU only):
    n tokens chosen one position at a time from seeded random candidates, keeping a candidate when
    its row's router gap in the fp32 reference is at least GAP in every layer (causal model: later
    tokens do not change earlier rows)."""
    rng = np.random.default_rng(seed)
    kv = PagedKVCache(CFG.num_layers, cpu.Hkv, CFG.head_dim, num_blocks=4, device="cpu", dtype=torch.float32)
    assert kv.blocks.reserve(1, n)
    bt = torch.from_numpy(kv.block_table([1]))
    toks = []
    for t in range(n):
        for _ in range(200):
            cand = int(rng.integers(0, CFG.vocab_size))
            with _RouterSpy() as spy:
                cpu.decode(torch.tensor([cand]), torch.tensor([t], dtype=torch.int32),
                           torch.from_numpy(kv.slots(1, t, 1)), kv, bt, torch.tensor([t + 1], dtype=torch.int32))
            if spy.min_gap(CFG.num_experts_per_tok) >= GAP:
                break
        else:
            raise AssertionError(f"no candidate with a router gap >= {GAP} at position {t}")
        toks.append(cand)
    return toks


def _reference_model():
    cpu = LLM(CFG, dtype=torch.float32, device="cpu")
    cpu.random_init(WEIGHTS)
    cpu.load_state_dict({k: v.bfloat16().float() for k, v in cpu.state_dict().items()})
    return cpu


@pytest.fixture(scope="module")
def pair():
    """An fp32 CPU model and a bf16 GPU model holding the same (bf16-valued) tensors, and token
    sequences built from the CPU model alone (:func:`_build_tokens`, kept in GOLDEN; every test
    asserts the margin they were built for): one of 70 tokens for the prefills, five of 24 + 3 b
    prompt tokens + 8 steps for decode and verify."""
    cpu = _reference_model()
    gpu = LLM(CFG, device=DEV)
    sd = gpu.state_dict()
    gpu.load_state_dict({k: v.to(sd[k].dtype) for k, v in cpu.state_dict().items()})
    for lc, lg in zip(cpu.layers, gpu.layers):
        assert lg.gu_w.shape == (CFG.num_experts, 2 * CFG.moe_intermediate_size, CFG.hidden_size)
        assert torch.equal(lg.router_w.float().cpu(), lc.router_w) and torch.equal(lg.gu_w.float().cpu(), lc.gu_w)
    tokens = json.loads(GOLDEN.read_text())
    seqs = {"prefill": tokens["prefill"], **{b: tokens[str(b)] for b in range(5)}}
    assert len(seqs["prefill"]) == 70 and all(len(seqs[b]) == 24 + 3 * b + 8 for b in range(5))
    return cpu, gpu, seqs


@pytest.mark.parametrize("T", [40, 70])
def test_prefill_matches_cpu_reference(pair, T):
    cpu, gpu, seqs = pair
    ids = torch.tensor(seqs["prefill"][:T])
    with _RouterSpy() as rc:
        ref = cpu.prefill(cpu.embed_tokens(ids))
    with _RouterSpy() as rg:
        got = gpu.prefill(gpu.embed_tokens(ids.to(DEV)))
    assert not gpu.norm_folded and rg.calls == CFG.num_layers
    _margin(rc, rg, f"prefill T = {T}")
    assert _cos(got, ref) > 0.99, _cos(got, ref)


def _prefilled(m, dev, seqs, B):
    kv = PagedKVCache(CFG.num_layers, m.Hkv, CFG.head_dim, num_blocks=16, device=dev,
                      dtype=torch.float32 if dev == "cpu" else torch.bfloat16)
    lens = [24 + 3 * b for b in range(B)]
    for b, T in enumerate(lens):
        kv.blocks.reserve(b + 1, T + 8)
        m.prefill(m.embed_tokens(torch.tensor(seqs[b][:T]).to(dev)), kv, torch.from_numpy(kv.slots(b + 1, 0, T)).to(dev))
    return kv, lens


def _step_args(kv, lens, step, ids, dev):
    B = len(lens)
    pos = torch.tensor([T + step for T in lens], dtype=torch.int32, device=dev)
    slots = torch.cat([torch.from_numpy(kv.slots(b + 1, lens[b] + step, 1)) for b in range(B)]).to(dev)
    bt = torch.from_numpy(kv.block_table([b + 1 for b in range(B)])).to(dev)
    return ids.to(dev), pos, slots, kv, bt, pos + 1


@pytest.mark.parametrize("B", [1, 5])
def test_decode_matches_cpu_reference(pair, B):
    """8 teacher-forced decode steps through a paged KV cache."""
    cpu, gpu, seqs = pair
    with _RouterSpy() as rc:
        kc, lens = _prefilled(cpu, "cpu", seqs, B)
        refs = [cpu.decode(*_step_args(kc, lens, s, torch.tensor([seqs[b][lens[b] + s] for b in range(B)]), "cpu"))
                for s in range(8)]
    with _RouterSpy() as rg:
        kg, _ = _prefilled(gpu, DEV, seqs, B)
        gots = [gpu.decode(*_step_args(kg, lens, s, torch.tensor([seqs[b][lens[b] + s] for b in range(B)]), DEV))
                for s in range(8)]
    _margin(rc, rg, f"decode B = {B}")
    for s in range(8):
        for b in range(B):
            assert _cos(gots[s][b], refs[s][b]) > 0.99, (s, b, _cos(gots[s][b], refs[s][b]))


def test_verify_matches_cpu_decode(pair):
    """LLM.verify with T = 4 against the CPU model's decode logits at the same positions."""
    cpu, gpu, seqs = pair
    T = 4
    with _RouterSpy() as rc:
        kc, lens = _prefilled(cpu, "cpu", seqs, 1)
        P = lens[0]
        refs = [cpu.decode(*_step_args(kc, lens, i, torch.tensor(seqs[0][P + i:P + i + 1]), "cpu")) for i in range(T)]
    with _RouterSpy() as rg:
        kg, _ = _prefilled(gpu, DEV, seqs, 1)
        ver = gpu.verify(torch.tensor(seqs[0][P:P + T], device=DEV), torch.arange(P, P + T, dtype=torch.int32, device=DEV),
                         torch.from_numpy(kg.slots(1, P, T)).to(DEV), kg, torch.from_numpy(kg.block_table([1])).to(DEV),
                         torch.tensor([P + T], dtype=torch.int32, device=DEV),
                         torch.tensor([T], dtype=torch.int32, device=DEV), T)
    assert ver.shape == (T, gpu.Vl)
    _margin(rc, rg, "verify T = 4")
    for i in range(T):
        assert _cos(ver[i], refs[i][0]) > 0.99, (i, _cos(ver[i], refs[i][0]))


def test_decode_graph_replay_is_bit_identical(pair):
    _, gpu, seqs = pair
    kv, lens = _prefilled(gpu, DEV, seqs, 1)
    args = _step_args(kv, lens, 0, torch.tensor([seqs[0][lens[0]]]), DEV)
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
    assert torch.equal(outs[0], eager), "same kernels, same order: the replay gives the eager bits"


def _generate(m, prompt, use_graphs):
    kv = PagedKVCache(CFG.num_layers, m.Hkv, CFG.head_dim, num_blocks=48, device=DEV, dtype=torch.bfloat16)
    eng = LLMEngine(m, kv, lambda ids: m.embed_tokens(torch.tensor(ids, device=DEV)), max_batch=4, use_graphs=use_graphs)
    try:
        r = eng.submit(prompt, len(prompt), SamplingParams(max_new_tokens=24), prompt_ids=prompt)
        for _ in r.stream(timeout=120):
            pass
        n_graphs = len(eng.graphs.graphs) if use_graphs else 0
        return list(r.tokens), n_graphs
    finally:
        eng.close()


def test_engine_with_graphs_keeps_the_tokens(pair):
    """24 greedy tokens with decode graphs on equal those with graphs off: the same kernels, and
    every one of them deterministic."""
    _, gpu, seqs = pair
    prompt = seqs[0][:24]
    base, _ = _generate(gpu, prompt, False)
    toks, n_graphs = _generate(gpu, prompt, True)
    assert len(base) == 24 and toks == base
    assert n_graphs >= 1, "no decode graph was captured"


if __name__ == "__main__":
    ref = _reference_model()
    built = {"prefill": _build_tokens(ref, 70, 0), **{str(b): _build_tokens(ref, 24 + 3 * b + 8, 10 + b) for b in range(5)}}
    GOLDEN.write_text(json.dumps(built) + "\n")
    print(f"wrote {GOLDEN}")
