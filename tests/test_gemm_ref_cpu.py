"""tests/gemm_ref.py against the fp32 CPU path of ops.linear / ops.linear_lnf, the exact range of every
integer case of tests/test_gemm_edges_gpu.py, and planted defects: each wrong output a GEMM kernel could
plausibly produce must fail its checker -- and the older one-number Frobenius criterion is shown to
pass several of them, which is the gap those GPU tests close."""
import pytest
import torch

import gemm_ref as G
from lumen_amd import ops

SMALL = G.RAGGED + G.INTERIOR
BF16, F32 = torch.bfloat16, torch.float32


def _out_dtype(spec):
    return F32 if spec.get("out_f32") else BF16


# --------------------------------------------------------------------------- reference vs the CPU path
@pytest.mark.parametrize("M,N,K", SMALL + G.DEEP_LDS128 + G.SKINNY_DEEP + [G.SKINNY_WIDE])
def test_ref64_agrees_with_cpu_path(M, N, K):
    """Every epilogue, random values, on every small, interior, deep-K and skinny table shape (the many-tile
    and tail-split shapes run with integer values only, on the GPU as well: see the exact test below)."""
    case = G.rand_inputs(M, N, K)
    worst = 0.0
    for name, spec in G.INT_EPILOGUES.items():
        ref = G.ref64(case.x, case.w, **G.epi_ref_kwargs(case, spec))
        buf, view, orow = G.run_linear(ops.linear, case, spec)
        G.assert_untouched(buf, view, rows=orow, what=name)
        worst = max(worst, G.check_elements(view[orow], ref.y, ref.mag, K, _out_dtype(spec), ref.actv, what=name))
    spec = G.INT_EPILOGUES["bias_res"]
    for act in G.ELEM_ACTS:
        ref = G.ref64(case.x, case.w, **{**G.epi_ref_kwargs(case, spec), "act": act})
        buf, view, orow = G.run_linear(ops.linear, case, spec, act=act)
        worst = max(worst, G.check_elements(view, ref.y, ref.mag, K, BF16, ref.actv, what=act))
    ref = G.ref64(case.x, case.w, bias=case.bias, glu=True)
    buf, view, _ = G.run_linear(ops.linear, case, G.INT_EPILOGUES["bias_bf16"], glu=True)
    G.assert_untouched(buf, view, what="glu")
    worst = max(worst, G.check_elements(view, ref.y, ref.mag, K, BF16, ref.actv, what="glu"))
    print(f"worst ratio to the bound ({M}, {N}, {K}): {worst:.3f}")


@pytest.mark.parametrize("M,N,K", SMALL)
@pytest.mark.parametrize("act", [None, "quick_gelu"])
def test_ref64_lnf_agrees_with_cpu_path(M, N, K, act):
    x, w, b, gam, bet = G.lnf_inputs(M, N, K)
    wf, ca = ops.ln_fold_weights(w, b, gam, bet)
    st = ops.ln_row_stats(x, 1e-5)
    ref = G.ref64_lnf(x, wf, ca, st, act)
    got = ops.linear_lnf(x, wf, ca, st, act=act)
    print(f"worst ratio: {G.check_elements(got, ref.y, ref.mag, K, BF16, ref.actv):.3f}")
    # and the folded form is LayerNorm + Linear: loose, the fold's own tests are elsewhere
    plain = ops.linear(ops.layer_norm(x.float(), gam.float(), bet.float(), 1e-5), w.float(), b.float(), act=act)
    assert G.frobenius_rel(got, plain) < 1e-2


# --------------------------------------------------------------------------- the integer cases are exact
INT_TABLE = ([(s, tuple(G.INT_EPILOGUES)) for s in SMALL]
             + [(s, G.DEEP_EPILOGUES) for s in G.DEEP_LDS128 + G.SKINNY_DEEP + [G.SKINNY_WIDE]]
             + [(s, G.BIG_EPILOGUES) for s in G.MANY_TILES + G.TAIL_SPLIT])


@pytest.mark.parametrize("shape,epis", INT_TABLE, ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else None)
def test_integer_cases_exact_on_cpu_path(shape, epis):
    """The builder's assertions hold (inside int_ref) and the fp32 CPU path reproduces the float64 reference
    bit for bit: the cases sit inside the exact range and ref64 applies the operations in the kernel's order."""
    case = G.int_inputs(*shape)
    top = 0.0
    for name in epis:
        ref = G.int_ref(*shape, name)
        buf, view, orow = G.run_linear(ops.linear, case, G.INT_EPILOGUES[name])
        G.assert_untouched(buf, view, rows=orow, what=name)
        G.check_exact(view[orow], ref.y, what=name)
        top = max(top, ref.y.abs().max().item())
    print(f"largest final value {shape}: {top:g}")


def test_skinny_interleaved_cases_in_exact_range():
    """The N = 16 calls that the skinny counter-reuse test puts between two calls of a table shape."""
    for M, _, K in G.SKINNY_DEEP + [G.SKINNY_WIDE]:
        G.int_ref(M, 16, K, "bias_relu_res_ldr")


def test_sparsity_rule_for_deep_k():
    """Dense x at K = 4096 leaves the range bf16 holds exactly; the 1024 / K rule keeps the sums inside it."""
    g = torch.Generator().manual_seed(0)
    x = torch.randint(-1, 2, (32, 4096), generator=g).double()
    w = torch.randint(-2, 3, (528, 4096), generator=g).double()
    assert (x @ w.t()).abs().max().item() > 256
    c = G.int_inputs(32, 528, 4096)
    assert (c.x.double() @ c.w.double().t()).abs().max().item() <= 256 - 8 - 16
    assert 0.2 < (c.x != 0).float().mean().item() < 0.3


def test_bound_is_tight_enough():
    """Median bound / |y| of the random-valued cases (those test_gemm_edges_gpu.py checks per element) is
    below 2^-6: an element off by one bias value (|b| ~ 1 against |y| ~ 1) cannot hide."""
    spec = G.INT_EPILOGUES["bias_res"]

    def rel(ref, K):
        return (G.elem_bound(ref.y, ref.mag, K, BF16, ref.actv) / ref.y.abs().clamp_min(1e-30)).median().item()

    for M, N, K in SMALL:
        case = G.rand_inputs(M, N, K)
        for act in (None,) + G.ELEM_ACTS:
            ref = G.ref64(case.x, case.w, **{**G.epi_ref_kwargs(case, spec), "act": act})
            assert rel(ref, K) < 2.0 ** -6, (M, N, K, act, rel(ref, K))
        ref = G.ref64(case.x, case.w, bias=case.bias, glu=True)
        assert rel(ref, K) < 2.0 ** -6, (M, N, K, "glu", rel(ref, K))
        x, w, b, gam, bet = G.lnf_inputs(M, N, K)
        wf, ca = ops.ln_fold_weights(w, b, gam, bet)
        for act in (None, "quick_gelu"):
            ref = G.ref64_lnf(x, wf, ca, ops.ln_row_stats(x, 1e-5), act)
            assert rel(ref, K) < 2.0 ** -6, (M, N, K, "lnf", act, rel(ref, K))


# --------------------------------------------------------------------------- planted defects
def _rne(y):
    return y.float().bfloat16()


def _trunc(y):
    return (y.float().view(torch.int32) & -65536).view(torch.float32).bfloat16()


def _exact(got, want, **_):
    G.check_exact(got, want)


def _defects():
    """name -> (got, want, check): ``got`` is what a kernel with the defect would leave in the [M, N] output,
    ``want`` the rounded reference (both for the Frobenius criterion), ``check`` runs the new checker."""
    out = {}
    M, N, K = 300, 272, 192
    c = G.int_inputs(M, N, K)
    x, w, b, r = c.x.double(), c.w.double(), c.bias.double(), c.residual.double()
    good = G.int_ref(M, N, K, "bias_res").y

    # bias shifted one column for n >= 256 (the ragged last column tile)
    b2 = b.clone()
    b2[256:] = b[255:-1]
    out["bias_shift_last_tile"] = (_rne(G.ref64(c.x, c.w, bias=b2, residual=c.residual).y), _rne(good), _exact)

    # out_group map: residual read at m instead of orow; table_offset dropped
    tg = G.int_ref(M, N, K, "table_group")
    kw = G.epi_ref_kwargs(c, G.INT_EPILOGUES["table_group"])
    acc = x @ w.t()
    t = c.table.double()[(torch.arange(M) % G.TAB_P) + G.TAB_OFF]
    out["residual_at_m"] = (_rne(acc + t + r[:M]), _rne(tg.y), _exact)
    out["table_offset_dropped"] = (_rne(G.ref64(c.x, c.w, **{**kw, "table_offset": 0}).y), _rne(tg.y), _exact)

    # accumulation: one 64-wide K-tile skipped for one 16x16 block (a many-tile case: one block among
    # 66560 x 256 elements); one K-tile counted twice for one 64-row slab
    Mb, Nb, Kb = G.MANY_TILES[0]
    cb = G.int_inputs(Mb, Nb, Kb)
    goodb = G.int_ref(Mb, Nb, Kb, "bias_res").y
    accb = cb.x.double() @ cb.w.double().t()
    a2 = accb.clone()
    a2[4112:4128, 32:48] -= cb.x.double()[4112:4128, 64:128] @ cb.w.double()[32:48, 64:128].t()
    out["k_tile_skipped_one_block"] = (_rne(G.ref64(cb.x, cb.w, bias=cb.bias, residual=cb.residual, acc=a2).y),
                                       _rne(goodb), _exact)
    a3 = acc.clone()
    a3[64:128] += x[64:128, 64:128] @ w[:, 64:128].t()
    out["k_tile_twice_one_slab"] = (_rne(G.ref64(c.x, c.w, bias=c.bias, residual=c.residual, acc=a3).y), _rne(good),
                                    _exact)

    # store: two 16-row slabs of a tile swapped
    sw = good.clone()
    sw[16:32], sw[32:48] = good[32:48], good[16:32]
    out["slabs_swapped"] = (_rne(sw), _rne(good), _exact)

    # order of the epilogue
    relu = G.int_ref(M, N, K, "bias_relu_res_ldr").y
    out["act_after_residual"] = (_rne((acc + b + r[:M]).clamp_min(0)), _rne(relu), _exact)
    two = G.int_ref(M, N, K, "alpha_two").y
    out["alpha_after_bias"] = (_rne(2.0 * (acc + b)), _rne(two), _exact)

    # bf16 store truncated instead of rounded (random values)
    cr = G.rand_inputs(M, N, K)
    rr = G.ref64(cr.x, cr.w, bias=cr.bias, act="gelu", residual=cr.residual)
    out["store_truncated"] = (_trunc(rr.y), _rne(rr.y),
                              lambda got, want, **_: G.check_elements(got, rr.y, rr.mag, K, BF16, rr.actv))

    # the last 16-column group of N = 272 not stored.  In a sentinel view the pattern remains; in the fresh
    # torch.empty of the older tests the caching allocator hands back the block the previous parametrised
    # case (same shape, same seed, another tile code) just freed, which holds the right values
    buf, view = G.sentinel_out(M, N, BF16)
    view[:, :256] = _rne(good)[:, :256]
    out["last_group_unstored"] = (_rne(good), _rne(good), lambda got, want, **_: G.check_exact(view, good))

    # row M written: outside what the older tests can see at all
    buf2, view2 = G.sentinel_out(M, N, BF16)
    view2.copy_(_rne(good))
    buf2[3 + M, 8:8 + N] = _rne(good)[M - 1]

    def stray(got, want, **_):
        G.check_exact(view2, good)
        G.assert_untouched(buf2, view2)
    out["row_M_written"] = (_rne(good), _rne(good), stray)

    # in-place residual read after the store of a 16-row slab: the stored value is added instead
    inp = G.int_ref(M, N, K, "inplace_res").y
    late = inp.clone()
    late[48:64] = (acc + b)[48:64] + inp[48:64]
    out["inplace_residual_read_late"] = (_rne(late), _rne(inp), _exact)
    return out


OLD_CRITERION_MUST_MISS = ("k_tile_skipped_one_block", "store_truncated", "last_group_unstored", "row_M_written")


def test_planted_defects_fail_their_checkers():
    defects = _defects()
    assert len(defects) == 12
    missed = []
    for name, (got, want, check) in defects.items():
        with pytest.raises(AssertionError):
            check(got, want)
        rel = G.frobenius_rel(got, want)
        if rel < 1e-2:
            missed.append(name)
        print(f"{name}: Frobenius ratio {rel:.2e} ({'passes' if rel < 1e-2 else 'fails'} the old criterion)")
    print("defects the old criterion (_rel < 1e-2) misses:", ", ".join(missed))
    for name in OLD_CRITERION_MUST_MISS:
        assert name in missed, name


def test_checkers_pass_the_undamaged_outputs():
    """The checkers used above are not trivially failing: the same outputs without a defect pass."""
    M, N, K = 300, 272, 192
    good = G.int_ref(M, N, K, "bias_res").y
    G.check_exact(_rne(good), good)
    G.check_exact(good.float(), good)
    buf, view = G.sentinel_out(M, N, BF16)
    view.copy_(_rne(good))
    G.assert_untouched(buf, view)
    cr = G.rand_inputs(M, N, K)
    rr = G.ref64(cr.x, cr.w, bias=cr.bias, act="gelu", residual=cr.residual)
    assert G.check_elements(_rne(rr.y), rr.y, rr.mag, K, BF16, rr.actv) <= 1.0
