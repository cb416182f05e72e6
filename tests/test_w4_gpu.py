"""4-bit group-quantised weight GEMMs (csrc/gemm_w4.hip) and the w4 decoder on the GPU.

The reference everywhere is the CPU path: an fp32 matmul over ``ops.dequantize_w4`` weights
(``ops.linear`` / ``ops.linear_dec`` with CPU tensors)."""
import pytest
import torch

from lumen_amd import ops
from lumen_amd.models.llm import LLM, LLM_PRESETS
from lumen_amd.runtime.kv_cache import PagedKVCache

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-6)).item()


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.float().cpu().flatten(), b.float().cpu().flatten(), dim=0).item()


def _w4(N, K, g, group=None):
    return ops.quantize_w4_rows(torch.randn(N, K, generator=g) * K ** -0.5, group)


# (M, N, K, G): the row-streaming GEMV (M <= 4, rows shorter than a wave step, a K tail), the MFMA
# skinny kernel (one and two row tiles, split K, a partial 128-wide block) and the prefill tile
# (ragged M); N no multiple of 64
@pytest.mark.parametrize("M,N,K,G", [(1, 64, 896, 32), (3, 48, 1024, 128), (5, 80, 896, 32), (16, 64, 2048, 128),
                                     (17, 48, 4864, 128), (32, 64, 1024, 32), (33, 96, 896, 128),
                                     (200, 192, 1024, 32)])
def test_gemm_w4_exact_integers(M, N, K, G):
    """Uniform codes, power-of-two group scales with wmin = -8 scale and small integer
    activations: every product and partial sum is exactly representable, so the fp32 output
    equals the CPU reference bit for bit whatever the summation order -- any nibble, k-order,
    group or fragment mix-up shows."""
    g = torch.Generator().manual_seed(M * 7 + N + K + G)
    codes = torch.randint(0, 16, (N, K), generator=g)
    scale = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (N, K // G), generator=g)]
    w4, params = ops.pack_w4(codes, scale, -8.0 * scale)
    x = torch.randint(-4, 5, (M, K), generator=g).bfloat16()
    ref = ops.linear(x.float(), w4, w_scale=params)
    got = ops.linear(x.to(DEV), w4.to(DEV), w_scale=params.to(DEV), out_dtype=torch.float32)
    assert got.dtype == torch.float32
    torch.testing.assert_close(got.cpu(), ref, rtol=0, atol=0)


@pytest.mark.parametrize("M,N,K", [(1, 896, 896), (4, 4864, 896), (16, 896, 4864), (30, 1024, 14336),
                                   (100, 1024, 4096), (624, 4096, 4096), (1, 28672, 4096)])
def test_gemm_w4_vs_dequantized(M, N, K):
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, K, generator=g).bfloat16()
    w4, p = _w4(N, K, g)
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g).bfloat16()
    ref = ops.linear(x.float(), w4, b, residual=r.float(), w_scale=p)
    got = ops.linear(x.to(DEV), w4.to(DEV), b.to(DEV), residual=r.to(DEV), w_scale=p.to(DEV))
    e16 = _rel(got, ref)
    ref32 = ops.linear(x.float(), w4, w_scale=p)
    got32 = ops.linear(x.to(DEV), w4.to(DEV), w_scale=p.to(DEV), out_dtype=torch.float32)
    e32 = _rel(got32, ref32)
    print(f"w4 {M}x{N}x{K}: rel bf16 {e16:.3e} fp32 {e32:.3e}")
    assert e16 < 1e-2
    assert got32.dtype == torch.float32 and e32 < 5e-3


@pytest.mark.parametrize("M", [3, 200])
def test_gemm_w4_swiglu(M):
    g = torch.Generator().manual_seed(M)
    I, K = 512, 896
    x = torch.randn(M, K, generator=g).bfloat16()
    gu = ops.glu_interleave(torch.randn(I, K, generator=g), torch.randn(I, K, generator=g)) * K ** -0.5
    w4, p = ops.quantize_w4_rows(gu)
    ref = ops.linear(x.float(), w4, glu=True, w_scale=p)
    got = ops.linear(x.to(DEV), w4.to(DEV), glu=True, w_scale=p.to(DEV))
    assert got.shape == (M, I) and _rel(got, ref) < 1e-2


@pytest.mark.parametrize("M", [1, 16])
def test_gemm_w4_glu_norm(M):
    """Wide-N decode GEMM through linear_dec: SwiGLU + folded RMSNorm (rstd computed from A)."""
    K, I = 1024, 14336
    g = torch.Generator().manual_seed(M + 5)
    x = (torch.randn(M, K, generator=g) * 2).bfloat16()
    w4, p = ops.quantize_w4_rows(ops.glu_interleave(torch.randn(I, K, generator=g) * K ** -0.5,
                                                    torch.randn(I, K, generator=g) * K ** -0.5))
    ref = ops.linear(ops.rms_norm(x.float(), torch.ones(K), 1e-5), w4, glu=True, w_scale=p)
    got = ops.linear_dec(x.to(DEV), w4.to(DEV), p.to(DEV), glu=True, norm_eps=1e-5)
    assert got.shape == (M, I) and _rel(got, ref) < 1e-2


def test_gemm_w4_chained_ssq():
    """A residual-producing GEMM writes the per-tile sums of squares (ssq_out) that the next,
    norm-folded GEMM turns into its rstd row scale (ssq_in), at M = 2."""
    M, K, Hd, N = 2, 1024, 896, 1152
    g = torch.Generator().manual_seed(9)
    a = torch.randn(M, K, generator=g).bfloat16()
    x0 = torch.randn(M, Hd, generator=g).bfloat16()
    w1, p1 = _w4(Hd, K, g)
    w2, p2 = _w4(N, Hd, g)
    # CPU: residual GEMM (bf16 residual stream), rms_norm (unit gamma), projection
    x1 = ops.linear(a.float(), w1, residual=x0.float(), w_scale=p1).bfloat16()
    ref = ops.linear(ops.rms_norm(x1.float(), torch.ones(Hd), 1e-5), w2, w_scale=p2)
    ssq = torch.zeros((32, Hd // 16), device=DEV, dtype=torch.float32)
    xd = x0.to(DEV).clone()
    ops.linear_dec(a.to(DEV), w1.to(DEV), p1.to(DEV), residual=xd, out=xd, ssq_out=ssq)
    assert _rel(xd, x1) < 1e-2
    torch.testing.assert_close(ssq[:M].sum(1).cpu(), xd.float().pow(2).sum(1).cpu(), rtol=1e-4, atol=0)
    got = ops.linear_dec(xd, w2.to(DEV), p2.to(DEV), norm_eps=1e-5, ssq_in=ssq)
    assert _rel(got, ref) < 1e-2


# ----------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def pair():
    """``tiny`` quantised on the CPU, and a GPU model holding the SAME codes, group parameters and
    other tensors: only the kernels differ."""
    cfg = LLM_PRESETS["tiny"]
    cpu = LLM(cfg, dtype=torch.float32, device="cpu")
    cpu.random_init(1)
    cpu.quantize_w4()
    gpu = LLM(cfg, device=DEV)
    gpu.quantize_w4()                       # same structure: uint8 weights + parameter buffers
    sd = gpu.state_dict()
    gpu.load_state_dict({k: v.to(sd[k].dtype) for k, v in cpu.state_dict().items()}, strict=False)
    for lc, lg in zip(cpu.layers, gpu.layers):
        for n in ("qkv", "o", "gu", "down"):
            getattr(lg, n + "_s").copy_(getattr(lc, n + "_s"))
            assert torch.equal(getattr(lg, n + "_w").cpu(), getattr(lc, n + "_w"))
    assert gpu.weight_dtype == "w4" and gpu.norm_folded and gpu.layers[0].qkv_w.dtype == torch.uint8
    return cfg, cpu, gpu


def test_llm_w4_prefill_matches_cpu_reference(pair):
    cfg, cpu, gpu = pair
    ids = torch.randint(0, cfg.vocab_size, (40,), generator=torch.Generator().manual_seed(11))
    ref = cpu.prefill(cpu.embed_tokens(ids))
    got = gpu.prefill(gpu.embed_tokens(ids.to(DEV)))
    assert _cos(got, ref) > 0.99, _cos(got, ref)


def _prefilled(m, cfg, dev, B, T0):
    """B sequences of T0 + 3 b prompt tokens prefilled into a fresh paged cache."""
    kv = PagedKVCache(cfg.num_layers, m.Hkv, cfg.head_dim, num_blocks=16, device=dev,
                      dtype=torch.float32 if dev == "cpu" else torch.bfloat16)
    lens = [T0 + 3 * b for b in range(B)]
    for b, T in enumerate(lens):
        ids = torch.randint(0, cfg.vocab_size, (T,), generator=torch.Generator().manual_seed(20 + b))
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
def test_llm_w4_decode_matches_cpu_reference(pair, B):
    """8 teacher-forced decode steps through a paged KV cache: the row-streaming GEMV (B = 1)
    and the MFMA skinny kernel (B = 5) with the folded-norm ssq chain."""
    cfg, cpu, gpu = pair
    steps = torch.randint(0, cfg.vocab_size, (8, B), generator=torch.Generator().manual_seed(30 + B))
    kc, lens = _prefilled(cpu, cfg, "cpu", B, 40)
    kg, _ = _prefilled(gpu, cfg, DEV, B, 40)
    for s in range(8):
        ref = cpu.decode(*_step_args(kc, lens, s, steps[s], "cpu"))
        got = gpu.decode(*_step_args(kg, lens, s, steps[s], DEV))
        for b in range(B):
            assert _cos(got[b], ref[b]) > 0.99, (s, b, _cos(got[b], ref[b]))


def test_llm_w4_decode_graph_replay_is_bit_identical(pair):
    cfg, _, gpu = pair
    kv, lens = _prefilled(gpu, cfg, DEV, 1, 40)
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


def _vlm_service_w4(tmp_path, device, port):
    import json

    import numpy as np

    from lumen_amd.models.vlm import write_vlm_model
    from lumen_amd.resources.validator import config_from_dict
    from lumen_amd.services.vlm import GeneralFastVLMService
    from lumen_amd.utils.image import encode_jpeg

    write_vlm_model(tmp_path / "models" / "fastvlm-tiny", "fastvlm-tiny")
    cfg = {"metadata": {"version": "1.0.0", "region": "other", "cache_dir": str(tmp_path)},
           "deployment": {"mode": "single", "service": "vlm"}, "server": {"port": port, "host": "127.0.0.1"},
           "services": {"vlm": {"enabled": True, "package": "lumen_vlm",
                                "import_info": {"registry_class": "lumen_vlm.fastvlm.GeneralFastVLMService",
                                                "add_to_server": "lumen_vlm.proto.ml_service_pb2_grpc.add_InferenceServicer_to_server"},
                                "backend_settings": {"device": device},
                                "models": {"general": {"model": "fastvlm-tiny", "runtime": "onnx",
                                                       "precision": "w4"}}}}}
    s = GeneralFastVLMService.from_config(config_from_dict(cfg).services["vlm"], tmp_path)
    s.initialize()
    try:
        llm = s.backend.model.llm
        assert llm.weight_dtype == "w4" and llm.layers[0].qkv_w.dtype == torch.uint8
        img = encode_jpeg(np.random.default_rng(0).integers(0, 255, (50, 70, 3), dtype=np.uint8))
        body, _, meta = s.handle("vlm_generate", img, "image/jpeg", {"prompt": "Describe.", "max_new_tokens": "10"})
        assert json.loads(body)["generated_tokens"] == 10 and float(meta["ttft_ms"]) > 0
        return s.backend.get_info()
    finally:
        s.close()


def test_vlm_service_w4_gpu(tmp_path):
    """A VLM configured with precision ``w4`` serves vlm_generate end to end (random-init weights)."""
    assert list(_vlm_service_w4(tmp_path, "cuda", 50561).precisions) == ["bf16", "w4"]
