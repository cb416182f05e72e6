"""References, checkers, input builders and case tables for the dense bf16 GEMM family (csrc/gemm.hip,
gemm_pp.hip, gemm_epi.h, the bf16 form of the 128x128 LDS-DMA pipeline in gemm_f8.hip, gemm_skinny.hip).

Plain torch; nothing here imports lumen_amd or needs a GPU (the helpers that build or compare buffers
work on whatever device their tensors live on).

* :func:`ref64` / :func:`ref64_lnf` -- float64 value of ``epi(alpha * x @ w.T)`` in the order gemm_epi.h
  applies it, plus the magnitude the rounding-error bound of :func:`check_elements` scales with.
* :func:`check_exact` -- bit equality, for integer-valued cases whose every intermediate is exactly
  representable (:func:`int_inputs` asserts that): any accumulation order gives the same bits, so one
  wrong 16-column group, one dropped K-tile or a bias shifted by a column shows as a wrong element.
* :func:`check_elements` -- a per-element error bound for random-valued cases.
* :func:`sentinel_out` / :func:`assert_untouched` -- ``out=`` views inside a buffer of NaN patterns, so a
  store past ``M`` or ``N`` (or into a skipped row of an ``out_group`` map) is seen.
* the case tables of tests/test_gemm_edges_gpu.py, shared with tests/test_gemm_ref_cpu.py so that every
  GPU case is known to sit inside the exact range before it meets a kernel.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import torch

NAN_BF16 = 0x7FE5                 # quiet NaN patterns no kernel produces
NAN_F32 = 0x7FE5A5A5


# --------------------------------------------------------------------------- float64 reference
def act64(z: torch.Tensor, act) -> torch.Tensor:
    """The compiled activations in float64 (exact erf / tanh forms, as the CPU path of ops.linear)."""
    if act is None:
        return z
    if act == "relu":
        return z.clamp_min(0)
    if act == "gelu":
        return 0.5 * z * (1 + torch.erf(z / math.sqrt(2.0)))
    if act == "quick_gelu":
        return z * torch.sigmoid(1.702 * z)
    if act == "silu":
        return z * torch.sigmoid(z)
    if act == "gelu_tanh":
        return 0.5 * z * (1 + torch.tanh(math.sqrt(2 / math.pi) * (z + 0.044715 * z ** 3)))
    raise ValueError(act)


def out_rows(M, out_group=0, out_group_stride=0, out_row_offset=0) -> torch.Tensor:
    """Output row of every A row: the ``out_group`` map of gemm_epi.h (identity when out_group == 0)."""
    m = torch.arange(M)
    if out_group <= 0:
        return m
    return (m // out_group) * out_group_stride + out_row_offset + m % out_group


class Ref(NamedTuple):
    y: torch.Tensor          # float64 [M, NO], in A-row order: row m belongs at out[orow[m]]
    mag: torch.Tensor        # float64 [M, NO]: sum of the magnitudes of everything added into y
    actv: torch.Tensor       # float64 [M, NO]: the activation's value (0 where there is none)
    orow: torch.Tensor       # long [M]


def _d(t):
    return None if t is None else t.detach().cpu().double()


def ref64(x, w, bias=None, act=None, residual=None, table=None, table_period=0, table_offset=0, alpha=1.0,
          out_group=0, out_group_stride=0, out_row_offset=0, glu=False, acc=None, steps=None, want_mag=True) -> Ref:
    """float64 ``epi(alpha * x @ w.T)`` in the order gemm_epi.h applies it: (+bias) -> act ->
    (+table[(m % P) + off]) -> (+residual[orow]) -> store at orow; ``glu``: silu(gate) * up of the
    [gate 8 | up 8] column interleave after the bias, N / 2 columns, nothing else.

    ``mag = |alpha| * (|x| @ |w|.T) + |b| + |t| + |r|`` (for SwiGLU the sum of the gate's and the up's, times
    the other factor's size: the first-order error of the product).  ``acc``: use this [M, N] accumulator in
    place of x @ w.T (planted defects).  ``steps``: a list that receives every intermediate value."""
    xd, wd = _d(x), _d(w)
    M, N = xd.shape[0], wd.shape[0]
    a = xd @ wd.t() if acc is None else acc.double()
    v = a * alpha
    # want_mag=False (the exact cases need none): skip the second matrix product, mag is then meaningless
    mag = abs(alpha) * (xd.abs() @ wd.abs().t()) if want_mag else torch.zeros_like(v)
    inter = [a, v]
    if bias is not None:
        b = _d(bias)[:N]
        v = v + b
        mag = mag + b.abs()
        inter.append(v)
    orow = out_rows(M, out_group, out_group_stride, out_row_offset)
    if glu:
        g, u = v.view(M, N // 16, 2, 8)[:, :, 0].reshape(M, N // 2), v.view(M, N // 16, 2, 8)[:, :, 1].reshape(M, N // 2)
        mg, mu = mag.view(M, N // 16, 2, 8)[:, :, 0].reshape(M, N // 2), mag.view(M, N // 16, 2, 8)[:, :, 1].reshape(M, N // 2)
        s = act64(g, "silu")
        y = s * u
        # d(silu)/dg <= 1.1: errors of g scaled by |u|, errors of u by |silu(g)|
        return Ref(y, 1.1 * mg * u.abs() + mu * s.abs(), y, orow)
    actv = torch.zeros_like(v)
    if act is not None:
        v = act64(v, act)
        actv = v
        inter.append(v)
    if table is not None:
        t = _d(table)[(torch.arange(M) % table_period) + table_offset, :N]
        v = v + t
        mag = mag + t.abs()
        inter.append(v)
    if residual is not None:
        r = _d(residual)[orow, :N]
        v = v + r
        mag = mag + r.abs()
        inter.append(v)
    if steps is not None:
        steps.extend(inter)
    return Ref(v, mag, actv, orow)


def ref64_lnf(x, wf, col_aff, row_aff, act=None) -> Ref:
    """float64 ``act(rstd * acc + (-mean * rstd) * colsum + bias')`` of ops.linear_lnf, from the very ``wf``,
    ``col_aff`` [2, N] and ``row_aff`` [M, 2] handed to the kernel (their producers have their own tests);
    ``mag = |rstd| * (|x| @ |wf|.T) + |ro * colsum| + |bias'|``."""
    xd, wd, ca, ra = _d(x), _d(wf), _d(col_aff), _d(row_aff)
    M = xd.shape[0]
    rs, ro = ra[:M, :1], ra[:M, 1:2]
    z = rs * (xd @ wd.t()) + ro * ca[0] + ca[1]
    mag = rs.abs() * (xd.abs() @ wd.abs().t()) + (ro * ca[0]).abs() + ca[1].abs()
    y = act64(z, act)
    return Ref(y, mag, y if act is not None else torch.zeros_like(y), torch.arange(M))


# --------------------------------------------------------------------------- checkers
def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def check_exact(got: torch.Tensor, y: torch.Tensor, what="") -> None:
    """Assert that ``got`` [M, N] (bf16 or fp32) holds ``y`` bit for bit (y rounded to got's type: the
    integer cases are exact in it, so the rounding changes nothing; -0 never occurs in them).  The message
    gives the first few (m, n, got, want), the number of wrong elements per 16x16 block and the
    256x256-tile coordinates they fall in."""
    g = got.detach().cpu()
    want = y.to(g.dtype)
    assert g.shape == want.shape, (g.shape, want.shape)
    bad = _bits(g) != _bits(want)
    if not bad.any():
        return
    idx = bad.nonzero()
    first = ", ".join(f"({int(m)}, {int(n)}): got {g[m, n].item()!r}, want {want[m, n].item()!r}" for m, n in idx[:6])
    blk, cnt = torch.unique(torch.stack([idx[:, 0] // 16, idx[:, 1] // 16], 1), dim=0, return_counts=True)
    blocks = ", ".join(f"block({int(b[0]) * 16}, {int(b[1]) * 16}): {int(c)}" for b, c in list(zip(blk, cnt))[:8])
    tiles = sorted({(int(m) // 256, int(n) // 256) for m, n in idx[:4096]})
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first {first}; "
                         f"{len(blk)} 16x16 blocks hit, {blocks}; 256-tiles (row, col) {tiles[:12]}")


def elem_bound(y, mag, K, out_dtype, actv=None) -> torch.Tensor:
    b = 1.25 * K * 2.0 ** -23 * mag + 1e-6
    if out_dtype == torch.bfloat16:
        b = b + 2.0 ** -8 * y.abs()
    if actv is not None:
        b = b + 2.0 ** -16 * actv.abs()
    return b


def check_elements(got, y, mag, K, out_dtype, actv=None, what="") -> float:
    """Assert, for every element (none is excluded; a NaN or inf in ``got`` fails),

        |got - y| <= 2^-8 * |y| + 1.25 * K * 2^-23 * mag + 2^-16 * |act value| + 1e-6

    (fp32 output: without the 2^-8 term) and return the worst ratio to the bound.  Where the terms come from:

    * the stores round to nearest (f2bf casts through __bf16): half a bf16 step, at most 2^-8 of |y|;
    * bf16 x bf16 products are exact in fp32;
    * any fp32 summation order of the K products (and the few epilogue terms) stays within
      (K - 1) * 2^-24 * sum|terms| of the exact sum; doubled to K * 2^-23, because the matrix core's
      internal accumulation need not round to nearest; sum|terms| is ``mag``;
    * that error passes through the activation, whose slope is at most 1.13 for the compiled
      activations: the factor 1.25;
    * 2^-16 of the activation's value covers the fast exp and reciprocal over |z| <= 16;
    * 1e-6 absorbs underflow next to zero.

    SwiGLU (``ref64(glu=True)``) is a product, y = silu(g) * u, of two such sums, so its ``mag`` is the
    first-order error of the product, ``1.1 * mag_g * |u| + mag_u * |silu(g)|``: an error e_g of the gate
    moves y by at most |silu'| * |u| * e_g with |silu'| <= 1.1, an error e_u of the up value by |silu(g)| * e_u
    (the second-order term e_g * e_u is below 2^-30 of these); e_g and e_u are the sums' errors above.  The
    constants of the bound itself are unchanged."""
    g = got.detach().cpu().double()
    assert g.shape == y.shape, (g.shape, y.shape)
    ratio = (g - y).abs() / elem_bound(y, mag, K, out_dtype, actv)
    ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, float("inf")))
    worst = ratio.max().item() if ratio.numel() else 0.0
    if not worst <= 1.0:
        m, n = (int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape))
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements over the bound; worst at "
                             f"({m}, {n}): got {g[m, n].item():.9g}, want {y[m, n].item():.9g}, mag "
                             f"{mag[m, n].item():.4g}, {worst:.3g} x the bound")
    return worst


def frobenius_rel(got, ref) -> float:
    """The one-number criterion of the older GEMM tests (they assert it is below 1e-2)."""
    a, b = got.float().cpu(), ref.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-6)).item()


# --------------------------------------------------------------------------- sentinel buffers
def sentinel_out(M, N, dtype, pad_rows=3, pad_cols=8, device="cpu"):
    """(buf, view): a buffer filled with a NaN bit pattern and the [M, N] view inside it, ``pad_rows`` spare
    rows above and below, ``pad_cols`` (a multiple of 8) spare columns left and right.  Row stride and column
    offset are multiples of 8 elements, so the view's rows are 16-byte aligned as every epilogue assumes."""
    assert pad_cols % 8 == 0 and dtype in (torch.bfloat16, torch.float32)
    ld = (N + 2 * pad_cols + 7) // 8 * 8
    it, pat = (torch.int16, NAN_BF16) if dtype == torch.bfloat16 else (torch.int32, NAN_F32)
    buf = torch.full((M + 2 * pad_rows, ld), pat, dtype=it, device=device).view(dtype)
    view = buf[pad_rows:pad_rows + M, pad_cols:pad_cols + N]
    assert view.stride(0) % 8 == 0 and view.data_ptr() % 16 == 0
    return buf, view


def assert_untouched(buf, view, rows=None, what="") -> None:
    """Every element of ``buf`` outside ``view`` (and, with ``rows``, inside the view but in none of these
    rows) still holds the sentinel, bit for bit."""
    ld = buf.stride(0)
    off = view.storage_offset() - buf.storage_offset()
    r0, c0 = off // ld, off % ld
    M, N = view.shape
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    if rows is None:
        keep[r0:r0 + M, c0:c0 + N] = False
    else:
        keep[r0 + rows.to(buf.device), c0:c0 + N] = False
    pat = NAN_BF16 if buf.dtype == torch.bfloat16 else NAN_F32
    bad = keep & (_bits(buf) != pat)
    if bad.any():
        idx = bad.nonzero()[:6].cpu()
        where = ", ".join(f"(row {int(r) - r0}, col {int(c) - c0})" for r, c in idx)
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the [{M}, {N}] output were written; first "
                             f"(relative to the view) {where}")


# --------------------------------------------------------------------------- inputs
class Case(NamedTuple):
    x: torch.Tensor
    w: torch.Tensor
    bias: torch.Tensor       # bf16 [N]; .float() is the fp32 form
    residual: torch.Tensor   # bf16 [rows of the scatter map's output, N]
    table: torch.Tensor      # bf16 [TAB_S, N]


TAB_P, TAB_S, TAB_OFF = 16, 17, 1          # the patch-rows-into-token-buffer map of the CLIP towers


def scatter_rows(M) -> int:
    """Rows of the output buffer under the (TAB_P, TAB_S, TAB_OFF) out_group map."""
    return int(out_rows(M, TAB_P, TAB_S, TAB_OFF)[-1]) + 1


@functools.lru_cache(maxsize=None)
def int_inputs(M, N, K, seed=0) -> Case:
    """Integer-valued operands: x from {-1, 0, 1} (for K > 1024 non-zero with probability 1024 / K, so a
    deep K does not push the sums past the exact range), w from {-2..2}, bias from {-8..8}, table and
    residual from {-16..16}.  :func:`int_ref` asserts the exactness of every epilogue built from them."""
    g = torch.Generator().manual_seed(seed * 7919 + M * 131 + N * 17 + K)
    if K > 1024:
        x = (2 * torch.randint(0, 2, (M, K), generator=g) - 1).float() * (torch.rand(M, K, generator=g) < 1024.0 / K)
    else:
        x = torch.randint(-1, 2, (M, K), generator=g).float()
    w = torch.randint(-2, 3, (N, K), generator=g).float()
    b = torch.randint(-8, 9, (N,), generator=g).float()
    t = torch.randint(-16, 17, (TAB_S, N), generator=g).float()
    r = torch.randint(-16, 17, (scatter_rows(M), N), generator=g).float()
    return Case(x.bfloat16(), w.bfloat16(), b.bfloat16(), r.bfloat16(), t.bfloat16())


@functools.lru_cache(maxsize=None)
def rand_inputs(M, N, K, seed=0) -> Case:
    """Random-valued operands in the recipe of the older tests: x = randn, w = randn / sqrt(K), the rest randn."""
    g = torch.Generator().manual_seed(seed * 7919 + M * 131 + N * 17 + K + 1)
    return Case(torch.randn(M, K, generator=g).bfloat16(), (torch.randn(N, K, generator=g) * K ** -0.5).bfloat16(),
                torch.randn(N, generator=g).bfloat16(), torch.randn(scatter_rows(M), N, generator=g).bfloat16(),
                torch.randn(TAB_S, N, generator=g).bfloat16())


# Epilogues of the exact tests: name -> (keywords of ops.linear / ref64 drawn from a Case, output type).
# "bias": "bf16" | "f32"; "residual": True (contiguous) | "ldr" (a column slice of a wider buffer) |
# "inplace" (the output buffer itself); "table": the (TAB_P, TAB_S, TAB_OFF) map; "strided": x and w as
# column slices of wider buffers (lda > K, ldw > K).
INT_EPILOGUES = {
    "plain": dict(),
    "bias_bf16": dict(bias="bf16"),
    "bias_f32": dict(bias="f32"),
    "bias_relu": dict(bias="bf16", act="relu"),
    "bias_res": dict(bias="bf16", residual=True),
    "bias_relu_res_ldr": dict(bias="bf16", act="relu", residual="ldr"),
    "alpha_half": dict(bias="bf16", alpha=0.5),
    "alpha_two": dict(bias="bf16", alpha=2.0),
    "f32_out": dict(bias="f32", residual=True, out_f32=True),
    "table_group": dict(table=True, residual=True),
    "inplace_res": dict(bias="bf16", residual="inplace"),
    "strided_xw": dict(bias="bf16", residual=True, strided=True),
}
# deep K: alpha stays at or below 1 (2 * 175 would leave the exact range)
DEEP_EPILOGUES = ("plain", "bias_relu_res_ldr", "alpha_half", "f32_out", "inplace_res")
BIG_EPILOGUES = ("bias_res", "inplace_res", "f32_out")              # the many-tile and tail-split tables


def epi_ref_kwargs(case: Case, spec: dict) -> dict:
    """ref64 keywords of an epilogue spec."""
    kw = {}
    if spec.get("bias"):
        kw["bias"] = case.bias
    if spec.get("act"):
        kw["act"] = spec["act"]
    if spec.get("alpha"):
        kw["alpha"] = spec["alpha"]
    if spec.get("residual"):
        kw["residual"] = case.residual
    if spec.get("table"):
        kw.update(table=case.table, table_period=TAB_P, table_offset=TAB_OFF, out_group=TAB_P,
                  out_group_stride=TAB_S, out_row_offset=TAB_OFF)
    return kw


@functools.lru_cache(maxsize=None)
def int_ref(M, N, K, epi, seed=0) -> Ref:
    """Reference of an integer case, with the builder's exactness assertions: every intermediate and the
    final value is an integer (a multiple of 1/2 under alpha = 0.5) of size <= 256 (<= 128 where a
    half-integer can occur) for a bf16 output -- 8 significand bits hold those exactly -- and below 2^24 for
    an fp32 one; the fp32 accumulator holds every partial sum in any order, those being bounded by
    |x| @ |w|.T <= 2 K < 2^24."""
    case, spec = int_inputs(M, N, K, seed), INT_EPILOGUES[epi]
    steps = []
    ref = ref64(case.x, case.w, steps=steps, want_mag=False, **epi_ref_kwargs(case, spec))
    lim = 2.0 ** 24 - 1 if spec.get("out_f32") else 256.0
    for v in steps:
        assert torch.equal(v * 2, torch.round(v * 2)), (M, N, K, epi, "not a multiple of 1/2")
        assert v.abs().max().item() <= lim, (M, N, K, epi, v.abs().max().item(), lim)
        odd = v[v != torch.round(v)]
        assert odd.numel() == 0 or odd.abs().max().item() <= lim / 2, (M, N, K, epi, odd.abs().max().item())
    assert 2 * K < 2 ** 24
    return ref


def _wide(t: torch.Tensor, device) -> torch.Tensor:
    """t as a column slice of a buffer 16 elements wider (row stride > width, 16-byte aligned base)."""
    buf = torch.zeros(t.shape[0], t.shape[1] + 16, dtype=t.dtype, device=device)
    buf[:, 8:8 + t.shape[1]] = t.to(device)
    return buf[:, 8:8 + t.shape[1]]


def run_linear(linear, case: Case, spec: dict, tile=-1, device="cpu", glu=False, act=None):
    """Call ``linear`` (ops.linear) on an epilogue spec, writing into a :func:`sentinel_out` view.  Returns
    (buf, view, orow): the output rows are ``view[orow]``.  ``act`` overrides the spec's activation."""
    M, N = case.x.shape[0], case.w.shape[0]
    dev = lambda t: t.to(device)
    x, w = (_wide(case.x, device), _wide(case.w, device)) if spec.get("strided") else (dev(case.x), dev(case.w))
    kw = dict(tile=tile, act=act or spec.get("act"), alpha=spec.get("alpha", 1.0), glu=glu)
    if spec.get("bias"):
        kw["bias"] = dev(case.bias.float() if spec["bias"] == "f32" else case.bias)
    rows, orow = M, torch.arange(M)
    if spec.get("table"):
        rows, orow = scatter_rows(M), out_rows(M, TAB_P, TAB_S, TAB_OFF)
        kw.update(table=dev(case.table), table_period=TAB_P, table_offset=TAB_OFF, out_group=TAB_P,
                  out_group_stride=TAB_S, out_row_offset=TAB_OFF)
    buf, view = sentinel_out(rows, N // 2 if glu else N, torch.float32 if spec.get("out_f32") else torch.bfloat16,
                             device=device)
    res = spec.get("residual")
    if res == "inplace":
        view.copy_(dev(case.residual[:rows]))
        kw["residual"] = view
    elif res == "ldr":
        kw["residual"] = _wide(case.residual[:rows], device)
    elif res:
        kw["residual"] = dev(case.residual[:rows])
    linear(x, w, out=view, **kw)
    return buf, view, orow


# --------------------------------------------------------------------------- case tables
RAGGED = [(1, 16, 64), (17, 48, 64), (33, 80, 128), (130, 144, 192), (300, 272, 192), (257, 528, 320)]
INTERIOR = [(512, 512, 128), (768, 256, 192), (512, 768, 64)]
DEEP_LDS128 = [(130, 144, 3072), (130, 144, 4096)]                       # tile 20000: S = 6 and S = 8
SKINNY_M = (1, 7, 16, 17, 32)
SKINNY_DEEP = [(M, 528, K) for M in SKINNY_M for K in (1600, 2624, 4096)]  # last K split of 320 / 64 / full
SKINNY_WIDE = (32, 4096, 512)                                            # 256 column tiles: unsplit
MANY_TILES = [(66560, 256, 128), (66637, 256, 128)]
TAIL_SPLIT = [(16 * 256 + 300, 4096, K) for K in (128, 256, 512)]        # 128x128 fallback, S = 2, S = 4

TILE_CODES = ([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 104, 204, 304, 245, 109, 209, 609, 709, 809, 909,
               1629, 1709, 1829, 1839, 1929, 1939, 17, 47, 48, 1007, 1008, 20000, 20002, 20003, 20005]
              + list(range(20011, 20026)) + [-1])
PERSISTENT_CODES = [7, 17, 47, 1007, 109, 709, 909, 1709, 1929, 1939]
TAIL_CODES = [4, 5, 6, 7, 8, 9, 245, 609, 709, 839, 939]
TAIL_CODES = TAIL_CODES + [1000 + c for c in TAIL_CODES]
PINGPONG_CODES = [9, 109, 209, 609, 709, 809, 909, 1629, 1709, 1829, 1839, 1929, 1939, -1]

ELEM_ACTS = ("gelu", "quick_gelu", "silu", "gelu_tanh")


def lnf_inputs(M, N, K, seed=0):
    """(x, w, bias, gamma, beta) of a folded-LayerNorm case: rows with a mean (0.5) and a spread (2) that make
    rstd * acc and -mean * rstd * colsum cancel, as in tests/test_kernels_gpu.py."""
    g = torch.Generator().manual_seed(seed * 7919 + M * 131 + N * 17 + K + 2)
    x = (torch.randn(M, K, generator=g) * 2 + 0.5).bfloat16()
    gam, bet = (torch.rand(K, generator=g) + 0.5).bfloat16(), (torch.randn(K, generator=g) * 0.1).bfloat16()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).bfloat16()
    return x, w, torch.randn(N, generator=g).bfloat16(), gam, bet
