"""The dense bf16 GEMM family (csrc/gemm.hip, gemm_pp.hip, gemm_epi.h, the bf16 form of the 128x128 LDS-DMA
pipeline of gemm_f8.hip, gemm_skinny.hip) at its edges, every output element checked against
tests/gemm_ref.py -- never against another GPU call:

* integer-valued operands whose every intermediate is exactly representable: the output must equal the
  float64 reference bit for bit, whatever the tile walk, split or accumulation order;
* random-valued operands under a per-element rounding-error bound (activations, SwiGLU, folded LayerNorm);
* every call writes into a view of a buffer of NaN patterns with spare rows and columns, which must stay
  untouched; residuals in place, strided operands, alpha, the out_group row map.

tests/test_gemm_ref_cpu.py proves on the CPU that every integer case sits inside the exact range and that
the checkers catch planted defects.  Each test prints its worst ratio to the bound ("RATIO family value")."""
import pytest
import torch

import gemm_ref as G
from lumen_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


def family(tile, M):
    """Kernel family of a tile code, as gemm_bf16 decodes it: the 256x256 LDS-DMA kernels by their epilogue
    digit, the ping-pong kernels by their variant digit (8 / 9: direct-store epilogue)."""
    if M <= 32 and tile in (-1, 9):
        return "skinny"
    if tile >= 20000:
        return "lds128"
    if tile < 0:
        return "auto"
    cfg, digit = tile % 10, (tile % 1000) // 100
    if 4 <= cfg <= 6:
        return f"glds-epi{digit}"
    if cfg == 9:
        return "pingpong-direct" if digit >= 8 else "pingpong-persistent" if digit & 1 else "pingpong"
    return {7: "persistent", 8: "ring"}.get(cfg, "register")


def _exact(shape, tile, epis):
    case = G.int_inputs(*shape)
    for name in epis:
        ref = G.int_ref(*shape, name)
        buf, view, orow = G.run_linear(ops.linear, case, G.INT_EPILOGUES[name], tile=tile, device=DEV)
        what = f"{shape} tile {tile} {name}"
        G.assert_untouched(buf, view, rows=orow, what=what)
        G.check_exact(view[orow.to(DEV)], ref.y, what=what)


# --------------------------------------------------------------------------- exact integer products
@pytest.mark.parametrize("tile", G.TILE_CODES)
@pytest.mark.parametrize("shape", G.RAGGED + G.INTERIOR, ids=lambda s: "x".join(map(str, s)))
def test_exact_small_and_interior(shape, tile):
    _exact(shape, tile, tuple(G.INT_EPILOGUES))


@pytest.mark.parametrize("shape", G.DEEP_LDS128, ids=lambda s: "x".join(map(str, s)))
def test_exact_deep_k_splits(shape):
    """The 128x128 pipeline's split over gridDim.y with S = 6 (K = 3072) and S = 8 (K = 4096)."""
    _exact(shape, 20000, G.DEEP_EPILOGUES)


@pytest.mark.parametrize("tile", G.PERSISTENT_CODES)
@pytest.mark.parametrize("shape", G.MANY_TILES, ids=lambda s: "x".join(map(str, s)))
def test_exact_many_tiles_per_workgroup(shape, tile):
    _exact(shape, tile, G.BIG_EPILOGUES)


@pytest.mark.parametrize("tile", G.TAIL_CODES)
@pytest.mark.parametrize("shape", G.TAIL_SPLIT, ids=lambda s: "x".join(map(str, s)))
def test_exact_tail_round_split(shape, tile):
    """16 full row tiles on the 256x256 kernel + 300 tail rows: the 128x128 fallback (K = 128), the split-K
    tail with S = 2 and S = 4 (K = 256, 512); codes + 1000 run the same shape unsplit."""
    _exact(shape, tile, G.BIG_EPILOGUES)


@pytest.mark.parametrize("shape", G.SKINNY_DEEP + [G.SKINNY_WIDE], ids=lambda s: "x".join(map(str, s)))
def test_exact_skinny_split_k_and_counter_reuse(shape):
    """Split-K with a short last chunk, and the arrival counters shared between back-to-back calls of
    different N: the shape twice, once with N = 16, once more."""
    M, N, K = shape
    _exact(shape, -1, G.DEEP_EPILOGUES)
    case, spec = G.int_inputs(*shape), G.INT_EPILOGUES["bias_relu_res_ldr"]
    ref = G.int_ref(*shape, "bias_relu_res_ldr")
    views = []
    for s in (shape, shape, (M, 16, K), shape):
        c, r = (case, ref) if s == shape else (G.int_inputs(*s), G.int_ref(*s, "bias_relu_res_ldr"))
        buf, view, _ = G.run_linear(ops.linear, c, spec, device=DEV)
        G.assert_untouched(buf, view, what=f"{s}")
        G.check_exact(view, r.y, what=f"{s}")
        views.append(view)
    assert torch.equal(views[0].view(torch.int16), views[1].view(torch.int16))


# --------------------------------------------------------------------------- per-element bounds
_cache = {}


def _act_ref(shape, act):
    if ("act", shape, act) not in _cache:
        case = G.rand_inputs(*shape)
        _cache["act", shape, act] = G.ref64(case.x, case.w, bias=case.bias, act=act, residual=case.residual)
    return _cache["act", shape, act]


def _glu_ref(shape):
    if ("glu", shape) not in _cache:
        case = G.rand_inputs(*shape)
        _cache["glu", shape] = G.ref64(case.x, case.w, bias=case.bias, glu=True)
    return _cache["glu", shape]


def _lnf_case(shape):
    """Device operands of a folded-LayerNorm case and, per activation, the reference built from the very
    wf / col_aff / row_aff tensors the kernel gets."""
    if ("lnf", shape) not in _cache:
        x, w, b, gam, bet = (t.to(DEV) for t in G.lnf_inputs(*shape))
        wf, ca = ops.ln_fold_weights(w, b, gam, bet)
        st = ops.ln_row_stats(x, 1e-5)
        refs = {act: G.ref64_lnf(x, wf, ca, st, act) for act in (None, "quick_gelu")}
        _cache["lnf", shape] = (x, wf, ca, st, refs)
    return _cache["lnf", shape]


@pytest.mark.parametrize("tile", G.TILE_CODES)
@pytest.mark.parametrize("shape", G.RAGGED + G.INTERIOR, ids=lambda s: "x".join(map(str, s)))
def test_elements_activations_and_swiglu(shape, tile):
    M, N, K = shape
    case, spec = G.rand_inputs(*shape), G.INT_EPILOGUES["bias_res"]
    worst = 0.0
    for act in G.ELEM_ACTS:
        ref = _act_ref(shape, act)
        buf, view, _ = G.run_linear(ops.linear, case, spec, tile=tile, device=DEV, act=act)
        G.assert_untouched(buf, view, what=f"{shape} tile {tile} {act}")
        worst = max(worst, G.check_elements(view, ref.y, ref.mag, K, BF16, ref.actv, what=f"{shape} tile {tile} {act}"))
    ref = _glu_ref(shape)
    buf, view, _ = G.run_linear(ops.linear, case, G.INT_EPILOGUES["bias_bf16"], tile=tile, device=DEV, glu=True)
    G.assert_untouched(buf, view, what=f"{shape} tile {tile} glu")
    worst = max(worst, G.check_elements(view, ref.y, ref.mag, K, BF16, ref.actv, what=f"{shape} tile {tile} glu"))
    print(f"RATIO {family(tile, M)} {worst:.4f}")


@pytest.mark.parametrize("tile", G.PINGPONG_CODES)
@pytest.mark.parametrize("shape", G.RAGGED + G.INTERIOR, ids=lambda s: "x".join(map(str, s)))
def test_elements_layernorm_folded(shape, tile):
    M, N, K = shape
    x, wf, ca, st, refs = _lnf_case(shape)
    worst = 0.0
    for act, ref in refs.items():
        buf, view = G.sentinel_out(M, N, BF16, device=DEV)
        ops.linear_lnf(x, wf, ca, st, act=act, out=view, tile=tile)
        G.assert_untouched(buf, view, what=f"{shape} tile {tile} lnf {act}")
        worst = max(worst, G.check_elements(view, ref.y, ref.mag, K, BF16, ref.actv, what=f"{shape} tile {tile} lnf {act}"))
    print(f"RATIO lnf-{family(tile, 33)} {worst:.4f}")


# --------------------------------------------------------------------------- host-side alignment check
def test_misaligned_out_is_refused_on_the_host():
    """Every epilogue stores 16 bytes at a time: an ``out`` whose rows are not 16-byte aligned is an error
    raised before any launch (the output keeps its fill)."""
    x = torch.zeros(16, 64, device=DEV, dtype=BF16)
    w = torch.zeros(64, 64, device=DEV, dtype=BF16)
    for dtype, width, off in ((BF16, 68, 0), (BF16, 72, 4), (F32, 66, 0), (F32, 68, 2)):
        buf = torch.full((16, width), 7.0, device=DEV, dtype=dtype)
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            ops.linear(x, w, out=buf[:, off:off + 64], tile=2)
        torch.cuda.synchronize()
        assert bool((buf == 7.0).all())
