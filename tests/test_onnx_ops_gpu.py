"""Element-wise tests of the ONNX node kernels (csrc/onnx_ops.hip: ew_binary, ew_unary,
softmax_rows, resize_bilinear_nhwc, bmm) and of the executor's routing to them, against the float64
reference of tests/onnx_ref.py.  Every output element is compared, never a norm.

Tolerances (derived from the number formats, not tuned):

* bf16 output:  |got - ref| <= 2^-8 * S + 1e-6, S = |ref| for element-wise ops and the sum of the
  absolute contributions for reductions / blends (one bf16 rounding, 2^-9, plus f32 arithmetic).
* f32 output of exact-arithmetic ops:  <= (K + 2) * 2^-23 * S, K the reduction length (1 for
  element-wise ops).
* f32 output of ops built on device math functions: MATH_TOL below, 4x the error measured on an
  MI355X against the float64 reference, never above 2^-10 relative (which keeps the bf16-rounded
  result within one bf16 ulp).  Elements with |ref| < 1e-3 are held to an absolute bound instead.
"""
import numpy as np
import pytest
import torch

import onnx_ref as R
from lumen_amd import ops
from lumen_amd.runtime.onnx_graph import OnnxGraph
from lumen_amd.utils import onnx_lite as ox

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DT = {"f32": F32, "bf16": BF16}
EPS_F32 = R.EPS_F32
REL_CEIL = 2.0 ** -10
ABS_CEIL = REL_CEIL * 1e-3
SMALL = 1e-3

# Worst error of the f32-output math-function ops over the inputs of this file, measured on an
# MI355X (gfx950) against the float64 reference: relative where |ref| >= 1e-3, absolute where
# |ref| < 1e-3 (0: the inputs give no element of that regime, so that bound is never applied).
#
#   op          kernel code                  measured rel   measured abs
#   sigmoid     1 / (1 + __expf(-v))         4.631e-07      3.211e-10
#   tanh        tanhf                        8.243e-08      1.646e-11
#   exp         __expf, |v| <= 100           3.395e-06      3.195e-10
#   log         __logf                       1.616e-07      0
#   sqrt        sqrtf                        5.762e-08      0
#   reciprocal  1.f / v                      5.914e-08      0
#   erf         erff                         9.511e-08      0
#   pow         powf                         1.215e-07      0
#   softmax     __expf, wave reductions      6.699e-07      6.018e-10
#
# The bounds are 4x the measured values (headroom for other inputs of the same range), capped at
# REL_CEIL / ABS_CEIL.  No op comes near the ceiling (2^-10 = 9.8e-4).
MATH_MEASURED = {
    "sigmoid": (4.631e-07, 3.211e-10), "tanh": (8.243e-08, 1.646e-11), "exp": (3.395e-06, 3.195e-10),
    "log": (1.616e-07, 0.0), "sqrt": (5.762e-08, 0.0), "reciprocal": (5.914e-08, 0.0), "erf": (9.511e-08, 0.0),
    "pow": (1.215e-07, 0.0), "softmax": (6.699e-07, 6.018e-10),
}
MATH_TOL = {k: (min(4 * r, REL_CEIL), min(4 * a, ABS_CEIL)) for k, (r, a) in MATH_MEASURED.items()}


def hip():
    return ops.hip_ops()


def gen(seed):
    return torch.Generator().manual_seed(seed)


to_np = R.f64
compare = R.compare


def out_range(ref, dtype):
    return R.out_range(ref, dtype == BF16)


def bound_for(ref, out_dtype, S=None, K=1, math_op=None):
    S = np.abs(ref) if S is None else S
    if out_dtype == BF16:
        return R.bound_bf16(S)
    if math_op is None:
        return R.bound_f32(S, K)
    rel, ab = MATH_TOL[math_op]
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(ref) >= SMALL, rel * np.abs(ref), ab)


def report_math(op, got_t, ref):
    """Print the measured error of a math-function op (f32 output) before it is asserted."""
    got, ref = to_np(got_t), np.asarray(ref, np.float64)
    fin = np.isfinite(ref) & np.isfinite(got)
    err, mag = np.abs(got[fin] - ref[fin]), np.abs(ref[fin])
    big = mag >= SMALL
    rel = float((err[big] / mag[big]).max()) if big.any() else 0.0
    ab = float(err[~big].max()) if (~big).any() else 0.0
    print(f"MEASURED {op} rel {rel:.3e} abs {ab:.3e}")


# =================================================================== ew_binary
def _views():
    """name -> (base shape of a, view of a, shape of b)."""
    return {
        "equal": ((3, 5, 7), lambda t: t, (3, 5, 7)),
        "bcast4": ((2, 1, 4, 1), lambda t: t, (1, 3, 1, 5)),
        "scalar_b": ((3, 5), lambda t: t, ()),
        "bcast6": ((2, 1, 3, 1, 2, 3), lambda t: t, (1, 2, 1, 2, 1, 3)),
        "a_transposed": ((7, 5, 3), lambda t: t.transpose(0, 2), (5, 1)),
        "a_offset_slice": ((4, 6), lambda t: t[:, 1:], (4, 5)),
        "numel1": ((1,), lambda t: t, (1,)),
        "numel255": ((255,), lambda t: t, (255,)),
        "numel256": ((256,), lambda t: t, (256,)),
        "numel257": ((257,), lambda t: t, (257,)),
    }


def _binary_inputs(opname, ashape, bshape, seed):
    """f32 CPU operand sets for one op: a list of (a, b)."""
    g = gen(seed)
    a = torch.randn(ashape, generator=g) * 2
    b = torch.randn(bshape, generator=g) * 2
    if opname == "div":                      # divisors bounded away from 0
        b = torch.where(b < 0, b - 0.5, b + 0.5)
        return [(a, b)]
    if opname == "pow":
        pos = a.abs() * 1.5 + 0.25           # positive bases, real exponents
        sel = torch.rand(bshape, generator=g) < 0.5
        e23 = torch.where(sel, torch.full(bshape, 2.0), torch.full(bshape, 3.0))
        return [(pos, b * 0.75), (-pos, e23)]       # negative bases, exponents 2.0 / 3.0 (LayerNorm's Pow(d, 2))
    return [(a, b)]


@pytest.mark.parametrize("group", list(_views()))
@pytest.mark.parametrize("op", range(7), ids=R.BINARY_OPS)
def test_ew_binary(op, group):
    opname = R.BINARY_OPS[op]
    ashape, view, bshape = _views()[group]
    for ai, (a32, b32) in enumerate(_binary_inputs(opname, ashape, bshape, 100 * op + len(group))):
        for an, adt in DT.items():
            for bn, bdt in DT.items():
                a_c, b_c = a32.to(adt), b32.to(bdt)
                av = view(a_c.to(DEV))
                bv = b_c.to(DEV)
                ref = R.binary(op, view(a_c), b_c)
                for on, odt in DT.items():
                    out = torch.full(ref.shape, 777.0, device=DEV, dtype=odt)
                    hip().ew_binary(av, bv, out, op)
                    r = out_range(ref, odt)
                    what = f"{opname}/{group}/set{ai}/{an},{bn}->{on}"
                    if opname == "pow" and odt == F32:
                        report_math("pow", out, r)
                    compare(out, r, bound_for(r, odt, math_op="pow" if opname == "pow" else None), what)


def test_ew_binary_b_strided_and_offset():
    """b as a non-contiguous view too (the two stride vectors are independent)."""
    g = gen(5)
    a = torch.randn(4, 5, generator=g)
    bb = torch.randn(5, 6, generator=g)
    for op in (0, 1, 3):
        b_c = torch.where(bb < 0, bb - 0.5, bb + 0.5)
        out = torch.empty(4, 5, device=DEV)
        hip().ew_binary(a.to(DEV), b_c.to(DEV)[:, 2:].t(), out, op)
        ref = R.binary(op, a, b_c[:, 2:].t())
        compare(out, ref, bound_for(ref, F32), f"op{op}")


def test_ew_binary_rejects_seven_dims_and_bad_op():
    a = torch.ones((1,) * 7, device=DEV)
    with pytest.raises(RuntimeError):
        hip().ew_binary(a, a, torch.empty((1,) * 7, device=DEV), 0)
    b = torch.ones(4, device=DEV)
    with pytest.raises(RuntimeError):
        hip().ew_binary(b, b, torch.empty(4, device=DEV), 7)


# =================================================================== ew_unary
MATH_UNARY = {"sigmoid", "tanh", "exp", "log", "sqrt", "reciprocal", "erf"}
POSITIVE_ONLY = {"log", "sqrt", "reciprocal"}
_SPECIAL = [0.0, -0.0, 100.0, -100.0, -0.5, 0.5, 1.0, -1.0, 2.0, -3.0, 3.0, -2.0, 7.0, -7.0, 64.0, -64.0, 1e-3,
            -1e-3, 2.5, -2.5, 80.0, -80.0, 6.0, -6.0, 0.25, 1.5, -1.5, 30.0, -30.0, 10.0, -10.0, 96.0]


def _unary_input(n, positive, seed):
    g = gen(seed)
    v = torch.cat([torch.tensor(_SPECIAL), (torch.rand(160, generator=g) - 0.5) * 16,
                   (torch.rand(80, generator=g) - 0.5) * 200])
    v = torch.roll(v, seed % 7)[:n]
    # exp() of 87..90 sits at the f32 / bf16 overflow edge, where inf-or-finite hangs on the last ulp
    v = torch.where((v.abs() > 87.0) & (v.abs() < 90.0), torch.sign(v) * 95.0, v)
    if positive:
        v = v.abs() + 2.0 ** -6
    return v


_UNARY_PARAMS = {"hardsigmoid": [(0.25, 0.375)], "leaky": [(0.125, 0.0)],
                 "clip": [(-float("inf"), 1.5), (-0.75, float("inf")), (-0.75, 1.5)]}


@pytest.mark.parametrize("op", range(17), ids=R.UNARY_OPS)
def test_ew_unary(op):
    name = R.UNARY_OPS[op]
    for n in (1, 255, 256, 257):
        v32 = _unary_input(n, name in POSITIVE_ONLY, 31 * op + n)
        for p0, p1 in _UNARY_PARAMS.get(name, [(0.0, 0.0)]):
            for in_n, idt in DT.items():
                x_c = v32.to(idt)
                ref = R.unary(op, x_c, p0, p1)
                for on, odt in DT.items():
                    out = torch.full((n,), 777.0, device=DEV, dtype=odt)
                    hip().ew_unary(x_c.to(DEV), out, op, p0, p1)
                    r = out_range(ref, odt)
                    math_op = name if name in MATH_UNARY else None
                    if math_op and odt == F32:
                        report_math(name, out, r)
                    compare(out, r, bound_for(r, odt, math_op=math_op), f"{name}/n{n}/{in_n}->{on}/p{p0},{p1}")


def test_ew_unary_identity_rounds_ties_to_even():
    u = 2.0 ** -8           # half a bf16 ulp at 1.0
    v = torch.tensor([1 + u, 1 + 3 * u, -(1 + u), -(1 + 3 * u), 1 + u + 2.0 ** -20, 1 + u - 2.0 ** -20, 2 + 2 * u,
                      2 + 6 * u, 0.5 + u / 2, 1 + 2 * u, 3.0e38, 1.0e-40], dtype=F32)
    out = torch.empty(v.numel(), device=DEV, dtype=BF16)
    hip().ew_unary(v.to(DEV), out, 16, 0.0, 0.0)
    ref = R.bf16_round(v.numpy())
    assert ref[0] == 1.0 and ref[1] == 1 + 4 * u and ref[2] == -1.0 and ref[4] == 1 + 2 * u and ref[5] == 1.0
    got = to_np(out)
    assert np.array_equal(got[:-1], ref[:-1]), (got, ref)
    assert got[-1] in (0.0, ref[-1])        # an f32 denormal may be flushed


def test_ew_unary_floor_ceil_exact():
    v = torch.tensor([-0.5, 0.5, -1.0, 1.0, 3.0, -3.0, 0.0, 2.5, -2.5, 1e6, -1e6, 0.999, -0.999])
    for op, f in ((13, np.floor), (14, np.ceil)):
        out = torch.empty(v.numel(), device=DEV)
        hip().ew_unary(v.to(DEV), out, op, 0.0, 0.0)
        assert np.array_equal(to_np(out), f(v.double().numpy()))


# =================================================================== softmax_rows
def _softmax_input(kind, rows, D, seed):
    x = torch.randn(rows, D, generator=gen(seed)) * 3
    if kind == "plus300":
        x = x + 300.0
    elif kind == "minus300":
        x = x - 300.0
    elif kind == "some_neg_inf" and D > 1:
        x[:, 1::3] = -float("inf")
    elif kind == "constant":
        x = torch.full((rows, D), 3.25) * torch.arange(1, rows + 1).view(-1, 1)
    return x


SOFTMAX_DTYPES = [(F32, F32), (BF16, BF16), (F32, BF16)]


def _check_softmax(x32, what):
    for idt, odt in SOFTMAX_DTYPES:
        x_c = x32.to(idt)
        out = torch.full(x_c.shape, 777.0, device=DEV, dtype=odt)
        hip().softmax_rows(x_c.to(DEV), out)
        ref = R.softmax(x_c)
        if odt == F32:
            report_math("softmax", out, ref)
        compare(out, ref, bound_for(ref, odt, math_op="softmax"), f"{what}/{idt}->{odt}")
        got = to_np(out)
        ninf = np.isneginf(to_np(x_c))
        assert np.all(got[ninf] == 0.0), what
        if odt == F32:
            D = x_c.shape[-1]
            assert np.all(np.abs(got.sum(axis=-1) - 1.0) <= D * EPS_F32), (what, got.sum(axis=-1))


@pytest.mark.parametrize("kind", ["plain", "plus300", "minus300", "some_neg_inf", "constant"])
@pytest.mark.parametrize("D", [1, 2, 63, 64, 65, 130, 1000])
def test_softmax_rows(D, kind):
    for rows in (1, 3, 4, 5):           # full and partial 4-row blocks
        _check_softmax(_softmax_input(kind, rows, D, 7 * D + rows), f"{kind}/rows{rows}/D{D}")


def test_softmax_rows_3d():
    _check_softmax(torch.randn(2, 3, 65, generator=gen(3)) * 3, "3d")


# =================================================================== resize_bilinear_nhwc
RESIZE_SHAPES = [((3, 5), (6, 10)), ((3, 5), (7, 8)), ((7, 9), (3, 4)), ((4, 6), (1, 1)), ((1, 1), (4, 4)),
                 ((5, 4), (5, 9)), ((2, 3), (1, 7))]


@pytest.mark.parametrize("src,dst", RESIZE_SHAPES, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("mode", range(4), ids=R.RESIZE_MODES)
def test_resize_bilinear_nhwc(mode, src, dst):
    for C in (8, 24):
        x = torch.randn(2, src[0], src[1], C, generator=gen(C + mode)).to(BF16)
        out = torch.full((2, dst[0], dst[1], C), 777.0, device=DEV, dtype=BF16)
        hip().resize_bilinear_nhwc(x.to(DEV), out, mode)
        ref, S = R.resize_bilinear_nhwc(x, dst[0], dst[1], mode)
        compare(out, ref, bound_for(ref, BF16, S), f"{R.RESIZE_MODES[mode]}/{src}->{dst}/C{C}")


# =================================================================== bmm
BMM_SHAPES = [(1, 1, 1, 1), (2, 16, 16, 16), (3, 17, 15, 33), (2, 5, 40, 7), (1, 33, 1, 100), (2, 3, 4, 0)]


def _check_bmm(a, b, c, a_ref, b_ref, what):
    hip().bmm(a, b, c)
    ref, S = R.bmm(a_ref, b_ref)
    K = a_ref.shape[-1]
    compare(c, ref, (K + 2) * EPS_F32 * S, what)
    if K == 0:
        assert not to_np(c).any()


@pytest.mark.parametrize("B,M,N,K", BMM_SHAPES)
def test_bmm(B, M, N, K):
    g = gen(B * 1000 + M * 100 + N * 10 + K)
    a32, b32 = torch.randn(B, M, K, generator=g), torch.randn(B, K, N, generator=g)
    for adt in (F32, BF16):                 # contiguous operands over the dtype grid
        for bdt in (F32, BF16):
            a_c, b_c = a32.to(adt), b32.to(bdt)
            c = torch.full((B, M, N), 777.0, device=DEV)
            _check_bmm(a_c.to(DEV), b_c.to(DEV), c, a_c, b_c, f"{adt},{bdt}")
    # b as k.transpose(-1, -2): the attention-score layout
    k_c = torch.randn(B, N, K, generator=g).to(BF16)
    c = torch.full((B, M, N), 777.0, device=DEV)
    _check_bmm(a32.to(DEV), k_c.to(DEV).transpose(-1, -2), c, a32, k_c.transpose(-1, -2), "b transposed")
    # a expanded along the batch (batch stride 0)
    a1 = torch.randn(1, M, K, generator=g)
    c = torch.full((B, M, N), 777.0, device=DEV)
    _check_bmm(a1.to(DEV).expand(B, M, K), b32.to(DEV), c, a1.expand(B, M, K), b32, "a expanded")
    # a sliced with a storage offset
    big = torch.randn(B, M + 1, K + 2, generator=g).to(BF16)
    c = torch.full((B, M, N), 777.0, device=DEV)
    _check_bmm(big.to(DEV)[:, 1:, 2:], b32.to(DEV), c, big[:, 1:, 2:], b32, "a sliced")
    # c as an interior slice of a sentinel-filled buffer
    buf = torch.full((B + 2, M + 2, N + 3), 777.0, device=DEV)
    _check_bmm(a32.to(DEV), b32.to(DEV), buf[1:B + 1, 1:M + 1, 2:N + 2], a32, b32, "c interior slice")
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[1:B + 1, 1:M + 1, 2:N + 2] = False
    assert bool((buf[mask] == 777.0).all()), "bmm wrote outside its output slice"


# =================================================================== wrapper checks
def test_onnx_wrappers_reject_host_outputs_and_bad_codes():
    x = torch.ones(2, 8, device=DEV)
    with pytest.raises(RuntimeError):
        hip().ew_unary(x, torch.empty(2, 8), 0, 0.0, 0.0)
    with pytest.raises(RuntimeError):
        hip().ew_unary(x, torch.empty(2, 8, device=DEV), 17, 0.0, 0.0)
    with pytest.raises(RuntimeError):
        hip().softmax_rows(x, torch.empty(2, 8))
    xb = torch.ones(1, 2, 2, 8, device=DEV, dtype=BF16)
    with pytest.raises(RuntimeError):
        hip().resize_bilinear_nhwc(xb, torch.empty(1, 4, 4, 8, dtype=BF16), 0)
    with pytest.raises(RuntimeError):
        hip().resize_bilinear_nhwc(xb, torch.empty(1, 4, 4, 8, device=DEV, dtype=BF16), 4)
    a = torch.ones(1, 2, 3, device=DEV)
    with pytest.raises(RuntimeError):
        hip().bmm(a, a.transpose(1, 2), torch.empty(1, 2, 2))


# =================================================================== executor routing
N_ = ox.Node


def _run_gpu(nodes, init, feeds, outputs=("y",)):
    g = ox.Graph(nodes, init, list(feeds), list(outputs))
    gpu = OnnxGraph(ox.write_model(g), device="cuda")
    assert gpu.fallback_nodes == []
    got = gpu.run({k: v.to(DEV) for k, v in feeds.items()})
    assert gpu.fallback_counts == {}, gpu.fallback_counts
    return got


def test_executor_softmax_axis1_4d():
    x = torch.randn(2, 5, 3, 4, generator=gen(1)) * 3
    got = _run_gpu([N_("Softmax", ["x"], ["y"], attrs={"axis": 1})], {}, {"x": x})[0]
    ref = R.softmax(x, 1)
    compare(got, ref, bound_for(ref, BF16), "softmax axis 1")


def test_executor_matmul_broadcast_leading_dims():
    g = gen(2)
    a, b = torch.randn(2, 1, 5, 7, generator=g), torch.randn(1, 3, 7, 4, generator=g)
    got = _run_gpu([N_("MatMul", ["a", "b"], ["y"])], {}, {"a": a, "b": b})[0]
    ref, S = R.bmm(a, b)
    compare(got, ref, bound_for(ref, BF16, S), "matmul")


@pytest.mark.parametrize("ctm", R.RESIZE_MODES)
def test_executor_resize_linear_modes(ctm):
    x = torch.randn(2, 3, 3, 5, generator=gen(3)).to(BF16).float()
    for dst in ((7, 8), (1, 1), (2, 10)):
        got = _run_gpu([N_("Resize", ["x", "", "", "sz"], ["y"],
                           attrs={"mode": "linear", "coordinate_transformation_mode": ctm})],
                       {"sz": np.array([2, 3, *dst], np.int64)}, {"x": x})[0]
        ref, S = R.resize_bilinear_nhwc(R.nhwc(to_np(x)), dst[0], dst[1], ctm)
        compare(got, R.nchw(ref), bound_for(ref, BF16, R.nchw(S)), f"{ctm}/{dst}")


def _dw_graph(prelu):
    g = gen(4)
    w = (torch.randn(8, 1, 3, 3, generator=g) * 0.5).to(BF16).float()
    b = torch.randn(8, generator=g)
    sl = (torch.rand(8, generator=g) * 0.5).to(BF16).float()
    x = torch.randn(2, 4, 7, 6, generator=g).to(BF16).float()
    nodes = [N_("Conv", ["x", "w", "b"], ["c" if prelu else "y"],
                attrs={"kernel_shape": [3, 3], "pads": [0, 0, 1, 1], "strides": [2, 2], "group": 4})]
    init = {"w": w.numpy(), "b": b.numpy()}
    if prelu:
        nodes.append(N_("PRelu", ["c", "sl"], ["y"]))
        init["sl"] = sl.numpy()
    xr = np.repeat(R.nhwc(to_np(x)), 2, axis=3)         # channel multiplier 2: output c reads input c // 2
    ref, S = R.depthwise_conv(xr, to_np(w).reshape(8, 3, 3).transpose(1, 2, 0), to_np(b), 2, 1, (0, 0, 1, 1))
    return nodes, init, x, ref, S, to_np(sl)


def test_executor_depthwise_conv_asymmetric_pads_multiplier():
    nodes, init, x, ref, S, _ = _dw_graph(False)
    got = _run_gpu(nodes, init, {"x": x})[0]
    compare(got, R.nchw(ref), R.nchw(bound_for(ref, BF16, S)), "depthwise conv")


def test_executor_prelu_after_depthwise_conv():
    """The conv result is rounded to bf16 before the PReLU kernels run and their result is rounded
    again; both roundings are at most 2^-9 of a value no larger than S, so 2^-8 * S still holds."""
    nodes, init, x, ref, S, sl = _dw_graph(True)
    got = _run_gpu(nodes, init, {"x": x})[0]
    ref = np.where(ref > 0, ref, ref * sl)
    compare(got, R.nchw(ref), R.nchw(bound_for(ref, BF16, S)), "depthwise conv + prelu")


def test_executor_variadic_max_min():
    g = gen(6)
    a, b, c = (torch.randn(2, 3, 4, generator=g) for _ in range(3))
    for op, f in (("Max", np.maximum), ("Min", np.minimum)):
        got = _run_gpu([N_(op, ["a", "b", "c"], ["y"])], {}, {"a": a, "b": b, "c": c})[0]
        ref = f(f(to_np(a), to_np(b)), to_np(c))
        compare(got, ref, bound_for(ref, BF16), op)
