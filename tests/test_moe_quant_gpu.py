"""fp8 and 4-bit experts in the grouped expert GEMMs (csrc/moe_wq.hip) on the GPU: one grouped GEMM per
format on exactly representable integers, bit for bit; the whole sparse MLP against the fp32 reference on
the same codes; aliasing, determinism and graph replay; then the quantised ``tiny-qwen3-moe`` decoder
(prefill, decode, verify, decode graphs, the engine) against the fp32 CPU model holding the same codes.

``python -m tests.test_moe_quant_gpu`` (repository root, CPU only) rebuilds the token sequences of
tests/golden/moe_quant_router_margin_tokens.json from the quantised CPU references."""
import json
from pathlib import Path

import pytest
import torch

from lumen_amd import ops
from lumen_amd.models.llm import LLM, LLM_PRESETS
from lumen_amd.ops import llm as lops
from tests.test_moe_gpu import (_RouterSpy, _build_tokens, _cos, _generate, _margin, _prefilled, _rel,
                                _step_args)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = LLM_PRESETS["tiny-qwen3-moe"]
QUANT = ["fp8", "w4"]

# (T, E, k, H, I), what it reaches
SHAPES = {
    "one-token": (1, 8, 2, 128, 64),             # w4 down is a half block, fp8 down a single k block
    "g128": (5, 16, 4, 256, 128),                # w4 G = 128 in both GEMMs
    "k-tail": (9, 8, 2, 1216, 64),               # fp8: one unrolled pass of 16 blocks + 3; w4: G = 32, partial last block
    "one-expert": (37, 4, 2, 128, 64),           # every first choice is expert 3: three ragged row blocks at MT = 1
    "prefill-tile": (300, 8, 2, 128, 64),        # 600 pairs, MT = 4
    "layer-width": (4, 16, 8, 2048, 768),        # the real K of both GEMMs, G = 128
}


# ------------------------------------------------------------------------------------------ exact integers
def _int_weights(fmt, E, N, K, g):
    """[E, N, K] integer-valued weights in format ``fmt`` -> (codes, scales): every value a small
    multiple of 0.25, so products with integer activations and all their partial sums are exact."""
    if fmt == "bf16":
        return torch.randint(-8, 9, (E, N, K), generator=g).bfloat16(), None
    pow2 = torch.tensor([0.25, 0.5, 1.0, 2.0])
    if fmt == "fp8":
        w = torch.randint(-8, 9, (E, N, K), generator=g).float().to(torch.float8_e4m3fn)
        return w, pow2[torch.randint(0, 4, (E, N), generator=g)].contiguous()
    G = ops.w4_group(K)
    codes = torch.randint(0, 16, (E * N, K), generator=g)
    scale = pow2[torch.randint(0, 4, (E * N, K // G), generator=g)]
    w4, params = ops.pack_w4(codes, scale, -8.0 * scale)
    return w4.view(E, N, K // 2), params.view(E, N, K // G, 2)


def _explicit_ids(name, T, E, k, g):
    ids = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).to(torch.int32)
    if name == "one-expert":
        ids[:, 1] = torch.where(ids[:, 0] == 3, ids[:, 1], ids[:, 0])
        ids[:, 0] = 3
    r = T // 2
    ids[r, k - 1] = E                            # a row whose ids include E and (k > 1, T > 1) -1
    if T > 1:
        ids[r, 0] = -1
    return ids


@pytest.mark.parametrize("fmt", ["bf16"] + QUANT)
@pytest.mark.parametrize("name", list(SHAPES))
def test_grouped_linear_exact_integers(name, fmt):
    """Integer activations in [-4, 4]; fp8 / bf16 codes integers in [-8, 8], 4-bit codes uniform in 0..15
    with wmin = -8 scale; power-of-two scales from {0.25 .. 2} per (expert, row) or group.  Every product
    and partial sum is a multiple of 0.25 below 2^24 quanta (K <= 2048: 4 * 16 * 2048 * 4 = 2^19), so the
    fp32 output equals the CPU reference bit for bit whatever the summation order: any nibble, k-order,
    group, scale, expert-stride or row-map mix-up shows.  Both GEMM geometries of the shape run:
    gate|up (N = 2I, K = H) and down (N = H, K = I)."""
    T, E, k, H, I = SHAPES[name]
    g = torch.Generator().manual_seed(1000 + 10 * list(SHAPES).index(name) + len(fmt))
    ids = _explicit_ids(name, T, E, k, g)
    for N, K in ((2 * I, H), (H, I)):
        x = torch.randint(-4, 5, (T, K), generator=g).bfloat16()
        w, s = _int_weights(fmt, E, N, K, g)
        ref = lops.moe_grouped_linear(x.float(), ids, w.float() if fmt == "bf16" else w, s)
        got = lops.moe_grouped_linear(x.to(DEV), ids.to(DEV), w.to(DEV), None if s is None else s.to(DEV))
        torch.cuda.synchronize()
        assert got.dtype == torch.float32 and got.shape == (T, k, N)
        torch.testing.assert_close(got.cpu(), ref, rtol=0, atol=0)
        bad = (ids < 0) | (ids >= E)
        assert bad.any() and not got.cpu()[bad].any(), "pairs with an id outside [0, E) come back zero"
        assert float(ref.abs().max()) > 0
    if T == 1:                                   # the row above held E only: -1 next to a valid id
        ids2 = torch.tensor([[-1, 5]], dtype=torch.int32)
        got = lops.moe_grouped_linear(x.to(DEV), ids2.to(DEV), w.to(DEV), None if s is None else s.to(DEV))
        ref = lops.moe_grouped_linear(x.float(), ids2, w.float() if fmt == "bf16" else w, s)
        torch.testing.assert_close(got.cpu(), ref, rtol=0, atol=0)
        assert not got[0, 0].any() and got[0, 1].any()


# ------------------------------------------------------------------------------------------ the whole MLP
_CASES = {}


def _quantize_experts(fmt, gu, down):
    q = ops.quantize_fp8_rows if fmt == "fp8" else ops.quantize_w4_rows
    out = []
    for w in (gu, down):
        E, N, K = w.shape
        c, s = q(w.reshape(E * N, K))
        out += [c.view(E, N, -1), s.view(E, N, *s.shape[1:])]
    return out[0], out[2], out[1], out[3]       # gu codes, down codes, gu_s, down_s


def _case(name, fmt):
    """Quantised expert tensors of a shape (made on the CPU, copied to the device) and -- computed once
    and shared, never modified -- the GPU's routing and the fp32 CPU reference on the GPU's own ids."""
    if (name, fmt) in _CASES:
        return _CASES[name, fmt]
    T, E, k, H, I = SHAPES[name]
    g = torch.Generator().manual_seed(200 + list(SHAPES).index(name))
    x = torch.randn(T, H, generator=g).bfloat16()
    gate_w = (torch.randn(E, H, generator=g) * 3.0 * H ** -0.5).bfloat16()
    if name == "one-expert":
        x[:, 0] = x[:, 0].abs() + 1.0
        gate_w[:, 0] = 0.0
        gate_w[3] = 0.0
        gate_w[3, 0] = 16.0
    # a factor per expert from {0.5, 1, 1.5, 2}, neighbours always different: whose scales were used shows
    fac = torch.tensor([0.5, 1.0, 1.5, 2.0])[(torch.arange(E) + int(torch.randint(0, 4, (1,), generator=g))) % 4]
    gu = torch.randn(E, 2 * I, H, generator=g) * H ** -0.5 * fac[:, None, None]
    down = torch.randn(E, H, I, generator=g) * I ** -0.5 * fac[:, None, None]
    gu_w, down_w, gu_s, down_s = _quantize_experts(fmt, gu, down)
    cpu = dict(x=x.float(), gate_w=gate_w.float(), gu_w=gu_w, down_w=down_w, gu_s=gu_s, down_s=down_s)
    c = dict(T=T, E=E, k=k, H=H, I=I, cpu=cpu, **{n: (x if n == "x" else gate_w if n == "gate_w" else cpu[n]).to(DEV)
                                                 for n in cpu})
    c["ids"], c["w"] = lops.moe_route(c["x"], c["gate_w"], k)
    c["ref"] = lops.moe_experts(cpu["x"], c["ids"].cpu(), c["w"].cpu(), gu_w, down_w, gu_s=gu_s, down_s=down_s)
    _CASES[name, fmt] = c
    return c


def _mlp(c, x=None, **kw):
    return lops.moe_mlp(c["x"] if x is None else x, c["gate_w"], c["gu_w"], c["down_w"], c["k"], gu_s=c["gu_s"],
                        down_s=c["down_s"], **kw)


@pytest.mark.parametrize("fmt", QUANT)
@pytest.mark.parametrize("name", list(SHAPES))
def test_mlp_and_experts_against_reference_on_gpu_ids(name, fmt):
    c = _case(name, fmt)
    ref, cpu = c["ref"], c["cpu"]
    got_e = lops.moe_experts(c["x"], c["ids"], c["w"], c["gu_w"], c["down_w"], gu_s=c["gu_s"], down_s=c["down_s"])
    got_m = _mlp(c)
    torch.cuda.synchronize()
    print(f"{name} {fmt}: rel experts {_rel(got_e, ref):.3e}, mlp {_rel(got_m, ref):.3e}")
    assert got_e.dtype == torch.bfloat16 and got_e.shape == ref.shape
    assert _rel(got_e, ref) < 1e-2
    assert _rel(got_m, ref) < 1e-2
    assert torch.equal(got_e, got_m), "moe_mlp is moe_route + moe_experts"
    if name == "one-expert":
        assert (c["ids"][:, 0] == 3).all()
    # control, on the reference alone: the next expert's scales / parameters move it by far more
    rolled = lops.moe_experts(cpu["x"], c["ids"].cpu(), c["w"].cpu(), cpu["gu_w"], cpu["down_w"],
                              gu_s=cpu["gu_s"].roll(1, 0).contiguous(), down_s=cpu["down_s"].roll(1, 0).contiguous())
    print(f"{name} {fmt}: reference moves by {_rel(rolled, ref):.3f} (scales of expert e - 1)")
    assert _rel(rolled, ref) > 5e-2


# ------------------------------------------------------------------------------------------ aliasing, determinism, graph
@pytest.mark.parametrize("fmt", QUANT)
def test_residual_aliasing_out(fmt):
    c = _case("one-expert", fmt)
    cpu = c["cpu"]
    res = (torch.randn(c["T"], c["H"], generator=torch.Generator().manual_seed(7)) * 0.3).bfloat16()
    ref = lops.moe_experts(cpu["x"], c["ids"].cpu(), c["w"].cpu(), cpu["gu_w"], cpu["down_w"], residual=res.float(),
                           gu_s=cpu["gu_s"], down_s=cpu["down_s"])
    buf = res.to(DEV).clone()
    out = _mlp(c, residual=buf, out=buf)
    assert out.data_ptr() == buf.data_ptr()
    sep = _mlp(c, residual=res.to(DEV))
    assert torch.equal(buf, sep), "in place and out of place agree bit for bit"
    assert _rel(buf, ref) < 1e-2
    assert _rel(c["ref"], ref) > 5e-2, "the residual is a visible part of the result"


@pytest.mark.parametrize("fmt", QUANT)
@pytest.mark.parametrize("name", ["g128", "prefill-tile"])
def test_two_eager_runs_are_bit_identical(name, fmt):
    c = _case(name, fmt)
    assert torch.equal(_mlp(c), _mlp(c))


@pytest.mark.parametrize("fmt", QUANT)
def test_graph_replay_follows_new_routing(fmt):
    """One captured graph serves any routing: overwrite the static input with rows that route
    differently, replay, and get the bits of an eager call on those rows."""
    c = _case("g128", fmt)
    x2 = c["x"].flip(1).contiguous()
    ids2, _ = lops.moe_route(x2, c["gate_w"], c["k"])
    assert not torch.equal(ids2, c["ids"]), "the second input must route differently"
    eager1, eager2 = _mlp(c), _mlp(c, x2)
    static_x = c["x"].clone()
    side = ops.private_stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _mlp(c, static_x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.CAPTURE_LOCK, torch.cuda.graph(graph, stream=side):
        cap = _mlp(c, static_x)
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
GOLDEN = Path(__file__).resolve().parent / "golden" / "moe_quant_router_margin_tokens.json"


def _reference_model(fmt):
    """fp32 CPU model with bf16-valued tensors, then quantised with its experts."""
    cpu = LLM(CFG, dtype=torch.float32, device="cpu")
    cpu.random_init(WEIGHTS)
    cpu.load_state_dict({k: v.bfloat16().float() for k, v in cpu.state_dict().items()})
    (cpu.quantize_fp8 if fmt == "fp8" else cpu.quantize_w4)(experts=True)
    return cpu


@pytest.fixture(scope="module", params=QUANT)
def pair(request):
    """A quantised fp32 CPU model and a GPU model holding the same codes, scales / parameters and other
    tensors (only the kernels differ), and the token sequences built from that CPU model alone
    (``_build_tokens`` of test_moe_gpu.py with its GAP; every test asserts the margin they were built for)."""
    fmt = request.param
    cpu = _reference_model(fmt)
    gpu = LLM(CFG, device=DEV)
    (gpu.quantize_fp8 if fmt == "fp8" else gpu.quantize_w4)(experts=True)     # same structure
    sd = gpu.state_dict()
    gpu.load_state_dict({k: v.to(sd[k].dtype) for k, v in cpu.state_dict().items()}, strict=False)
    for lc, lg in zip(cpu.layers, gpu.layers):
        for n in ("qkv", "o", "gu", "down"):
            getattr(lg, n + "_s").copy_(getattr(lc, n + "_s"))
            assert torch.equal(getattr(lg, n + "_w").cpu().view(torch.uint8), getattr(lc, n + "_w").view(torch.uint8))
        assert torch.equal(lg.router_w.float().cpu(), lc.router_w) and lg.router_w.dtype == torch.bfloat16
        assert lg.gu_w.dim() == 3 and lg.gu_s.shape[:2] == (CFG.num_experts, 2 * CFG.moe_intermediate_size)
    assert gpu.weight_dtype == fmt and not gpu.norm_folded and not gpu._f8_ok(4096)
    tokens = json.loads(GOLDEN.read_text())[fmt]
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
    _margin(rc, rg, f"{gpu.weight_dtype} prefill T = {T}")
    assert _cos(got, ref) > 0.99, _cos(got, ref)


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
    _margin(rc, rg, f"{gpu.weight_dtype} decode B = {B}")
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
    _margin(rc, rg, f"{gpu.weight_dtype} verify T = 4")
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


def test_engine_with_graphs_keeps_the_tokens(pair):
    """24 greedy tokens with decode graphs on equal those with graphs off."""
    _, gpu, seqs = pair
    prompt = seqs[0][:24]
    base, _ = _generate(gpu, prompt, False)
    toks, n_graphs = _generate(gpu, prompt, True)
    assert len(base) == 24 and toks == base
    assert n_graphs >= 1, "no decode graph was captured"


if __name__ == "__main__":
    built = {}
    for fmt in QUANT:
        ref = _reference_model(fmt)
        built[fmt] = {"prefill": _build_tokens(ref, 70, 0),
                      **{str(b): _build_tokens(ref, 24 + 3 * b + 8, 10 + b) for b in range(5)}}
    GOLDEN.write_text(json.dumps(built) + "\n")
    print(f"wrote {GOLDEN}")
