"""Element-wise tests of the small NHWC kernels of csrc/conv.hip (pool2d, global_avgpool,
upsample_add, channel_scale_, channel_affine, pixel_shuffle_up) and of both depthwise kernels
(the generic dw_conv_kernel and the register-blocked dw_conv_rb_kernel) against the float64
reference of tests/onnx_ref.py, with the tolerance rules of tests/test_onnx_ops_gpu.py:

* bf16 output:  |got - ref| <= 2^-8 * S + 1e-6   (S = |ref|, or the sum of absolute contributions)
* f32 output:   |got - ref| <= (K + 2) * 2^-23 * S   (K the reduction length)

and the argument checks of their host wrappers (csrc/ops.cpp).  Every rejection case errs on the
large side (a longer vector, a larger output, a wider dtype), so no launch could leave its tensors
even without the check.
"""
import numpy as np
import pytest
import torch

import onnx_ref as R
from lumen_amd import ops
from lumen_amd.ops import cnn

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16


def gen(seed):
    return torch.Generator().manual_seed(seed)


def hip():
    return ops.hip_ops()


def rnd(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=gen(seed)) * scale).to(BF16)


# =================================================================== pool2d
POOL_CFG = [(3, 2, 1), (2, 2, 0), ((3, 2), (2, 1), (1, 0))]


@pytest.mark.parametrize("k,s,p", POOL_CFG)
@pytest.mark.parametrize("hw", [(7, 5), (8, 8)])
@pytest.mark.parametrize("is_max", [True, False], ids=["max", "avg"])
def test_pool2d(is_max, hw, k, s, p):
    for C in (8, 24):
        x = rnd(2, hw[0], hw[1], C, seed=C + hw[0])
        if is_max:                      # all-negative input: padding that contributed 0 would win the max
            x = (-x.float().abs() - 0.5).to(BF16)
        got = cnn.pool2d(x.to(DEV), k, s, p, is_max)
        ref, S = R.pool2d(x, k, s, p, is_max, count_include_pad=True)
        R.compare(got, ref, R.bound_bf16(S), f"C{C}")
        if is_max:
            assert float(got.float().max()) < 0
        elif p != 0:                    # the border pixels are where count_include_pad shows
            excl, _ = R.pool2d(x, k, s, p, False, count_include_pad=False)
            assert np.any(np.abs(excl[:, 0, 0] - ref[:, 0, 0]) > 4 * R.bound_bf16(S)[:, 0, 0])


# =================================================================== global_avgpool
@pytest.mark.parametrize("C", [8, 64, 72, 136])
@pytest.mark.parametrize("hw", [(1, 1), (1, 3), (2, 2), (5, 1), (7, 7)], ids=lambda v: f"hw{v[0] * v[1]}")
def test_global_avgpool(hw, C):
    x = rnd(2, hw[0], hw[1], C, seed=C + hw[0] * hw[1]) + 0.5
    got = cnn.global_avgpool(x.to(DEV))
    assert got.dtype == F32
    ref, S = R.global_avgpool(x)
    R.compare(got, ref, R.bound_f32(S, hw[0] * hw[1]), f"C{C}")


# =================================================================== upsample_add
@pytest.mark.parametrize("f", [2, 3, 4])
@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
def test_upsample_add(with_add, f):
    x = rnd(2, 3, 2, 16, seed=f)
    add = rnd(2, 3 * f, 2 * f, 16, seed=f + 10) if with_add else None
    ref = R.upsample_add(x, f, add)
    S = ref if add is None else R.upsample_add(x.abs(), f, add.abs())
    got = cnn.upsample_add(x.to(DEV), add.to(DEV) if with_add else None, f)
    if with_add:
        R.compare(got, ref, R.bound_bf16(S), "contiguous")
    else:
        assert np.array_equal(R.f64(got), ref)
    # out as a channel slice of a wider buffer (pixel stride 40 instead of 16)
    buf = torch.full((2, 3 * f, 2 * f, 40), 777.0, device=DEV, dtype=BF16)
    cnn.upsample_add(x.to(DEV), add.to(DEV) if with_add else None, f, out=buf[..., 8:24])
    R.compare(buf[..., 8:24], ref, R.bound_bf16(S) if with_add else 0.0, "channel slice")
    assert bool((buf[..., :8] == 777.0).all()) and bool((buf[..., 24:] == 777.0).all())


# =================================================================== channel_scale_
def test_channel_scale_per_image():
    x = rnd(2, 5, 1, 24, seed=1)
    s = torch.rand(2, 24, generator=gen(2)) + 0.25
    s[1] = s[1] * 3 + 1             # the two images get clearly different scales
    ref = R.channel_scale(x, s)
    xg = x.clone().to(DEV)
    got = cnn.channel_scale_(xg, s.to(DEV))
    assert got.data_ptr() == xg.data_ptr()
    R.compare(got, ref, R.bound_bf16(np.abs(ref)), "channel_scale_")


# =================================================================== channel_affine
@pytest.mark.parametrize("prelu", [False, True], ids=["noprelu", "prelu"])
@pytest.mark.parametrize("act", list(range(10)), ids=R.ACTS)
def test_channel_affine(act, prelu):
    # rows * C/8 = 45, 182 and 612 threads: under one 256-thread block, and a partial third block
    for shape in ((1, 3, 5, 24), (2, 7, 13, 8), (2, 9, 17, 16)):
        C = shape[-1]
        g = gen(act * 10 + C)
        x = rnd(*shape, seed=act + C, scale=2.0)
        sc = torch.rand(C, generator=g) + 0.5
        sh = torch.randn(C, generator=g)
        pr = (torch.rand(C, generator=g) * 0.5).to(BF16) if prelu else None
        out = torch.full(shape, 777.0, device=DEV, dtype=BF16)
        hip().channel_affine(x.to(DEV), sc.to(DEV), sh.to(DEV), out, act, pr.to(DEV) if prelu else None)
        ref = R.channel_affine(x, sc, sh, act, pr)
        R.compare(out, ref, R.bound_bf16(np.abs(ref)), f"{R.ACTS[act]}/{shape}")


# =================================================================== pixel_shuffle_up
@pytest.mark.parametrize("f", [2, 4])
@pytest.mark.parametrize("C", [8, 16])
def test_pixel_shuffle_up_exact(C, f):
    y = rnd(2, 3, 2, f * f * C, seed=C + f)
    got = cnn.pixel_shuffle_up(y.to(DEV), C, f)
    assert np.array_equal(R.f64(got), R.depth_to_space(y, f))


# =================================================================== depthwise conv
def _dw_case(C, H, W, KH, KW, stride, pads, dil, bias_dt, out_dt, act=None, seed=0):
    g = gen(seed + 13 * KH + 7 * KW + C)
    x = torch.randn(2, H, W, C, generator=g).to(BF16)
    w = (torch.randn(KH, KW, C, generator=g) * 0.3).to(BF16)
    b = torch.randn(C, generator=g).to(bias_dt) if bias_dt is not None else None
    Ho, Wo = cnn.conv_out_hw(H, W, KH, KW, stride, pads, dil)
    assert Ho > 0 and Wo > 0
    out = torch.full((2, Ho, Wo, C), 777.0, device=DEV, dtype=out_dt)
    cnn.conv2d_dw(x.to(DEV), w.to(DEV), b.to(DEV) if b is not None else None, stride, pads, dil, act=act, out=out)
    ref, S = R.depthwise_conv(x, w, b, stride, dil, pads)
    if act == "relu":
        ref = np.maximum(ref, 0.0)
    assert ref.shape == (2, Ho, Wo, C)
    bound = R.bound_bf16(S) if out_dt == BF16 else R.bound_f32(S, KH * KW + 1)
    R.compare(out, ref, bound, f"C{C} {H}x{W} k{KH}x{KW} s{stride} p{pads} d{dil} {bias_dt}->{out_dt}")


# dispatch (csrc/conv.hip conv2d_depthwise): dilation 1, KW in {3, 5, 7} and stride_w in {1, 2} take the
# register-blocked kernel, everything else the generic one
DW_GENERIC = [
    # KH, KW, stride, pads, dilation
    (3, 3, 1, 2, 2),                    # dilation 2
    (3, 3, (1, 1), (2, 1, 2, 1), (2, 1)),   # dilation in h only
    (1, 1, 1, 0, 1),                    # K = 1
    (7, 1, 1, (3, 0, 3, 0), 1),
    (2, 2, 1, 0, 1),
    (2, 2, 2, (0, 0, 1, 1), 1),
    (3, 3, 3, 1, 1),                    # stride 3
    (3, 4, (2, 1), (1, 1, 1, 2), 1),    # stride (2, 1), even KW
    (3, 3, 2, (0, 0, 1, 1), 2),         # asymmetric pads + dilation
]
DW_RB = [
    (1, 7, 1, (0, 3, 0, 3), 1),
    (3, 5, 1, (1, 2, 1, 2), 1),
    (3, 3, (2, 1), 1, 1),               # sh != sw
    (3, 3, (1, 2), 1, 1),
    (5, 5, 2, 2, 1),
    (7, 7, 1, 3, 1),
    (3, 3, 2, (0, 0, 1, 1), 1),         # asymmetric pads
]


@pytest.mark.parametrize("KH,KW,stride,pads,dil", DW_GENERIC + DW_RB)
def test_depthwise_kernels(KH, KW, stride, pads, dil):
    for C in (8, 24):
        _dw_case(C, 9, 8, KH, KW, stride, pads, dil, BF16, BF16)
    _dw_case(24, 9, 8, KH, KW, stride, pads, dil, F32, F32, seed=1)      # the executor's f32 bias; f32 out
    _dw_case(8, 9, 8, KH, KW, stride, pads, dil, None, BF16, act="relu", seed=2)


@pytest.mark.parametrize("K,s", [(3, 1), (3, 2), (5, 1), (7, 1), (7, 2)])
@pytest.mark.parametrize("Wo", [1, 2, 3, 5])
def test_depthwise_rb_partial_pixel_groups(Wo, K, s):
    """Output rows of 1, 2, 3 and 5 pixels: partial 4-pixel groups of the register-blocked kernel."""
    W = (Wo - 1) * s + 1                 # with pad K // 2 this gives exactly Wo outputs
    _dw_case(16, 5, W, K, K, s, K // 2, 1, F32, BF16)
    _dw_case(16, 5, W, K, K, s, K // 2, 1, BF16, F32, seed=3)


def test_depthwise_input_narrower_than_kernel():
    for H, W in ((2, 2), (3, 2), (1, 1)):
        _dw_case(8, H, W, 7, 7, 1, 3, 1, F32, BF16)
        _dw_case(8, H, W, 7, 7, 1, 3, 1, F32, F32)


# =================================================================== wrapper checks
def _t(*shape, dt=BF16):
    return torch.ones(*shape, device=DEV, dtype=dt)


REJECT = {
    "channel_scale_ C % 8": lambda: hip().channel_scale_(_t(1, 2, 2, 12), _t(1, 12, dt=F32)),
    "channel_scale_ f32 x": lambda: hip().channel_scale_(_t(1, 2, 2, 8, dt=F32), _t(1, 8, dt=F32)),
    "channel_scale_ s length": lambda: hip().channel_scale_(_t(1, 2, 2, 8), _t(2, 8, dt=F32)),
    "pixel_shuffle_up y channels": lambda: hip().pixel_shuffle_up(_t(1, 2, 2, 40), _t(1, 4, 4, 8), 2),
    "pixel_shuffle_up C % 8": lambda: hip().pixel_shuffle_up(_t(1, 2, 2, 48), _t(1, 4, 4, 12), 2),
    "pixel_shuffle_up out shape": lambda: hip().pixel_shuffle_up(_t(1, 2, 2, 32), _t(1, 5, 4, 8), 2),
    "pixel_shuffle_up f32 y": lambda: hip().pixel_shuffle_up(_t(1, 2, 2, 32, dt=F32), _t(1, 4, 4, 8), 2),
    "pixel_shuffle_up f32 out": lambda: hip().pixel_shuffle_up(_t(1, 2, 2, 32), _t(1, 4, 4, 8, dt=F32), 2),
    "pool2d out shape": lambda: hip().pool2d(_t(1, 4, 4, 8), _t(1, 3, 3, 8), [2, 2], [2, 2], [0, 0], True),
    "pool2d out channels": lambda: hip().pool2d(_t(1, 4, 4, 8), _t(1, 2, 2, 16), [2, 2], [2, 2], [0, 0], True),
    "pool2d f32 x": lambda: hip().pool2d(_t(1, 4, 4, 8, dt=F32), _t(1, 2, 2, 8), [2, 2], [2, 2], [0, 0], True),
    "pool2d f32 out": lambda: hip().pool2d(_t(1, 4, 4, 8), _t(1, 2, 2, 8, dt=F32), [2, 2], [2, 2], [0, 0], False),
    "global_avgpool f32 x": lambda: hip().global_avgpool(_t(2, 2, 2, 8, dt=F32), _t(2, 8, dt=F32)),
    "global_avgpool out shape": lambda: hip().global_avgpool(_t(2, 2, 2, 8), _t(2, 16, dt=F32)),
    "upsample_add out shape": lambda: hip().upsample_add(_t(1, 2, 2, 8), None, _t(1, 5, 4, 8), 2),
    "upsample_add add shape": lambda: hip().upsample_add(_t(1, 2, 2, 8), _t(1, 5, 4, 8), _t(1, 4, 4, 8), 2),
    "upsample_add f32 x": lambda: hip().upsample_add(_t(1, 2, 2, 8, dt=F32), None, _t(1, 4, 4, 8), 2),
    "upsample_add f32 add": lambda: hip().upsample_add(_t(1, 2, 2, 8), _t(1, 4, 4, 8, dt=F32), _t(1, 4, 4, 8), 2),
    "channel_affine out shape": lambda: hip().channel_affine(_t(1, 2, 2, 8), _t(8, dt=F32), _t(8, dt=F32),
                                                            _t(1, 3, 2, 8), 0, None),
    "channel_affine f32 out": lambda: hip().channel_affine(_t(1, 2, 2, 8), _t(8, dt=F32), _t(8, dt=F32),
                                                          _t(1, 2, 2, 8, dt=F32), 0, None),
    "channel_affine f64 shift": lambda: hip().channel_affine(_t(1, 2, 2, 8), _t(8, dt=F32), _t(8, dt=torch.float64),
                                                            _t(1, 2, 2, 8), 0, None),
    "channel_affine scale length": lambda: hip().channel_affine(_t(1, 2, 2, 8), _t(16, dt=F32), _t(8, dt=F32),
                                                               _t(1, 2, 2, 8), 0, None),
    "channel_affine prelu length": lambda: hip().channel_affine(_t(1, 2, 2, 8), _t(8, dt=F32), _t(8, dt=F32),
                                                               _t(1, 2, 2, 8), 0, _t(16)),
    "channel_affine f32 prelu": lambda: hip().channel_affine(_t(1, 2, 2, 8), _t(8, dt=F32), _t(8, dt=F32),
                                                            _t(1, 2, 2, 8), 0, _t(8, dt=F32)),
    "conv2d_dw bias length": lambda: hip().conv2d_dw(_t(1, 4, 4, 8), _t(3, 3, 8), _t(16, dt=F32), 0, [1, 1], [1, 1],
                                                     [1, 1], _t(1, 4, 4, 8)),
    "conv2d_dw f16 bias": lambda: hip().conv2d_dw(_t(1, 4, 4, 8), _t(3, 3, 8), _t(8, dt=torch.float16), 0, [1, 1],
                                                  [1, 1], [1, 1], _t(1, 4, 4, 8)),
    "conv2d_dw f32 w": lambda: hip().conv2d_dw(_t(1, 4, 4, 8), _t(3, 3, 8, dt=F32), None, 0, [1, 1], [1, 1], [1, 1],
                                               _t(1, 4, 4, 8)),
    "conv2d_dw out batch": lambda: hip().conv2d_dw(_t(1, 4, 4, 8), _t(3, 3, 8), None, 0, [1, 1], [1, 1], [1, 1],
                                                   _t(2, 4, 4, 8)),
    "conv2d_dw f64 out": lambda: hip().conv2d_dw(_t(1, 4, 4, 8), _t(3, 3, 8), None, 0, [1, 1], [1, 1], [1, 1],
                                                 _t(1, 4, 4, 8, dt=torch.float64)),
}


@pytest.mark.parametrize("case", list(REJECT))
def test_wrapper_rejects(case):
    with pytest.raises(RuntimeError):
        REJECT[case]()
    torch.cuda.synchronize()
