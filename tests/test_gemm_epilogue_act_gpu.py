"""Direct-store ping-pong GEMM (tile codes 1839 / 1939): the activation is a compile-time parameter of
the epilogue (none / quick_gelu / gelu); any other activation is routed to the LDS-staged form of the
same tile code.  Every epilogue against the fp32 CPU reference of the same op."""
import functools

import pytest
import torch

from lumen_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

# several interior 256x256 tiles per launch; nk = 2 and nk = 3 (even / odd K-tile count of the two-phase loop)
SHAPES = [(512, 512, 128), (768, 256, 192)]
TILES = [1839, 1939]                          # direct-store: non-persistent (production), persistent
ACTS = [None, "quick_gelu", "gelu", "silu"]   # three compiled activations + one routed to the LDS-staged form


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-6)).item()


@functools.lru_cache(maxsize=None)
def _inputs(M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).bfloat16()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).bfloat16()
    b = torch.randn(N, generator=g).bfloat16()
    r = torch.randn(M, N, generator=g).bfloat16()
    xl = (torch.randn(M, K, generator=g) * 2 + 0.5).bfloat16()
    gam, bet = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.1
    return x, w, b, r, xl, gam, bet


@functools.lru_cache(maxsize=None)
def _refs(M, N, K, act):
    """fp32 CPU references of the four epilogues, computed once per (shape, activation)."""
    x, w, b, r, xl, gam, bet = _inputs(M, N, K)
    return {
        "plain": ops.linear(x, w, act=act),
        "bias": ops.linear(x, w, b, act=act),
        "bias_res": ops.linear(x, w, b, act=act, residual=r),
        "lnf": ops.linear(ops.layer_norm(xl.float(), gam, bet, 1e-5), w.float(), b.float(), act=act),
    }


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("act", ACTS)
def test_gemm_direct_store_activation(M, N, K, tile, act):
    x, w, b, r, xl, gam, bet = _inputs(M, N, K)
    ref = _refs(M, N, K, act)
    xd, wd, bd, rd = x.to(DEV), w.to(DEV), b.to(DEV), r.to(DEV)
    for name, kw in (("plain", {}), ("bias", {"bias": bd}), ("bias_res", {"bias": bd, "residual": rd})):
        got = ops.linear(xd, wd, act=act, tile=tile, **kw)
        assert torch.isfinite(got).all(), name
        assert _rel(got, ref[name]) < 1e-2, name
    wf, ca = ops.ln_fold_weights(wd, bd, gam.to(DEV).bfloat16(), bet.to(DEV).bfloat16())
    xld = xl.to(DEV)
    st = ops.ln_row_stats(xld, 1e-5)
    got = ops.linear_lnf(xld, wf, ca, st, act=act, tile=tile)
    assert torch.isfinite(got).all(), "lnf"
    assert _rel(got, ref["lnf"]) < 1e-2, "lnf"


@pytest.mark.parametrize("tile", TILES)
def test_gemm_direct_store_ragged_dispatch_unchanged(tile):
    """Rows outside the interior-tile fast path (M = 300) still take the generic epilogue."""
    M, N, K = 300, 512, 128
    x, w, b, r, _, _, _ = _inputs(M, N, K)
    ref = ops.linear(x, w, b, act="gelu", residual=r)
    got = ops.linear(x.to(DEV), w.to(DEV), b.to(DEV), act="gelu", residual=r.to(DEV), tile=tile)
    assert torch.isfinite(got).all()
    assert _rel(got, ref) < 1e-2
