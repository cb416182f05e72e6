"""tests/onnx_ref.py (the float64 reference the GPU element-wise tests compare against) vs torch's
float64 CPU ops wherever torch implements the same semantics, and vs hand-computed vectors for
the Resize coordinate modes torch does not have."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import onnx_ref as R

TOL = 1e-12
RNG = np.random.default_rng(7)


def _close(got, ref, tol=TOL):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref)
    assert np.all(err <= tol * np.maximum(1.0, np.abs(ref))), float(err.max())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------ resize
HW_PAIRS = [((3, 5), (6, 10)), ((3, 5), (7, 8)), ((7, 9), (3, 4)), ((4, 6), (1, 1)), ((1, 1), (4, 4)),
            ((5, 4), (5, 9)), ((2, 3), (1, 7))]


@pytest.mark.parametrize("src,dst", HW_PAIRS)
@pytest.mark.parametrize("mode,align", [("half_pixel", False), ("align_corners", True)])
def test_resize_matches_torch_interpolate(src, dst, mode, align):
    x = RNG.standard_normal((2, src[0], src[1], 3))
    y, S = R.resize_bilinear_nhwc(x, dst[0], dst[1], mode)
    ref = F.interpolate(_t(R.nchw(x)), size=dst, mode="bilinear", align_corners=align)
    _close(R.nchw(y), ref.numpy())
    refS = F.interpolate(_t(R.nchw(np.abs(x))), size=dst, mode="bilinear", align_corners=align)
    _close(R.nchw(S), refS.numpy())


def _resize_w(vals, wo, mode):
    x = np.asarray(vals, np.float64).reshape(1, 1, -1, 1)
    return R.resize_bilinear_nhwc(x, 1, wo, mode)[0].reshape(-1)


def test_resize_asymmetric_hand_vectors():
    _close(_resize_w([0, 1, 2, 3], 8, "asymmetric"), [0, .5, 1, 1.5, 2, 2.5, 3, 3])
    # 4 -> 3: x = o * 4/3 = 0, 1.333.., 2.666..
    _close(_resize_w([0, 10, 20, 30], 3, "asymmetric"), [0, 40 / 3, 80 / 3])
    # 4 -> 1: x = 0
    _close(_resize_w([5, 1, 2, 3], 1, "asymmetric"), [5])
    # 2 -> 5: x = 0, .4, .8, 1.2 -> clamp 1, 1.6 -> clamp 1
    _close(_resize_w([1, 2], 5, "asymmetric"), [1, 1.4, 1.8, 2, 2])


def test_resize_pytorch_half_pixel_hand_vectors():
    # a length-1 output samples coordinate 0, not the half-pixel centre
    _close(_resize_w([0, 1, 2, 3], 1, "pytorch_half_pixel"), [0.0])
    _close(_resize_w([0, 1, 2, 3], 1, "half_pixel"), [1.5])
    # any longer output is half_pixel: 4 -> 8 gives -.25 (clamped), .25, .75, ...
    hp = [0, .25, .75, 1.25, 1.75, 2.25, 2.75, 3]
    _close(_resize_w([0, 1, 2, 3], 8, "pytorch_half_pixel"), hp)
    _close(_resize_w([0, 1, 2, 3], 8, "half_pixel"), hp)
    # 4 -> 2: x = 0.5, 2.5
    _close(_resize_w([0, 1, 2, 3], 2, "pytorch_half_pixel"), [.5, 2.5])


def test_resize_align_corners_hand_vectors():
    _close(_resize_w([0, 1, 2, 3], 7, "align_corners"), [0, .5, 1, 1.5, 2, 2.5, 3])
    _close(_resize_w([4, 1, 2, 3], 1, "align_corners"), [4])


def test_resize_modes_differ_in_both_axes():
    """H and W take their own coordinate maps (a transposed input gives the transposed output)."""
    x = RNG.standard_normal((1, 3, 5, 2))
    for mode in R.RESIZE_MODES:
        y, _ = R.resize_bilinear_nhwc(x, 7, 4, mode)
        yt, _ = R.resize_bilinear_nhwc(x.transpose(0, 2, 1, 3), 4, 7, mode)
        _close(y, yt.transpose(0, 2, 1, 3))


# ------------------------------------------------------------------ elementwise / softmax / matmul
def test_unary_matches_torch():
    x = np.concatenate([RNG.standard_normal(200) * 3, [0.0, -0.0, 100.0, -100.0, -0.5, 2.0, -3.0]])
    pos = np.abs(x) + 0.01
    t = _t(x)
    fns = {"relu": F.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh, "exp": torch.exp, "neg": torch.neg,
           "abs": torch.abs, "hardswish": F.hardswish, "floor": torch.floor, "ceil": torch.ceil, "erf": torch.erf,
           "identity": lambda v: v}
    for name, f in fns.items():
        _close(R.unary(name, x), f(t).numpy())
    for name, f in {"log": torch.log, "sqrt": torch.sqrt, "reciprocal": torch.reciprocal}.items():
        _close(R.unary(name, pos), f(_t(pos)).numpy())
    _close(R.unary("leaky", x, 0.3), F.leaky_relu(t, 0.3).numpy())
    _close(R.unary("hardsigmoid", x, 0.25, 0.375), torch.clamp(t * 0.25 + 0.375, 0, 1).numpy())
    _close(R.unary("hardsigmoid", x, 1 / 6, 0.5), F.hardsigmoid(t).numpy())
    _close(R.unary("clip", x, -1.0, 2.0), torch.clamp(t, -1.0, 2.0).numpy())
    _close(R.unary("clip", x, -np.inf, 2.0), torch.clamp(t, max=2.0).numpy())
    _close(R.unary("clip", x, -1.0, np.inf), torch.clamp(t, min=-1.0).numpy())
    for code, name in enumerate(R.UNARY_OPS):       # codes and names address the same function
        arg = pos if name in ("log", "sqrt", "reciprocal") else x
        _close(R.unary(code, arg, 0.25, 0.375), R.unary(name, arg, 0.25, 0.375))


def test_acts_match_torch():
    x = np.concatenate([RNG.standard_normal(200) * 3, [0.0, -3.0, 3.0, -8.0, 8.0]])
    t = _t(x)
    fns = {"none": lambda v: v, "gelu": F.gelu, "quick_gelu": lambda v: v * torch.sigmoid(1.702 * v), "relu": F.relu,
           "silu": F.silu, "gelu_tanh": lambda v: F.gelu(v, approximate="tanh"), "hardswish": F.hardswish,
           "sigmoid": torch.sigmoid, "leaky": lambda v: F.leaky_relu(v, 0.1), "hardsigmoid": F.hardsigmoid}
    assert set(fns) == set(R.ACTS)
    for i, name in enumerate(R.ACTS):
        _close(R.act(name, x), fns[name](t).numpy())
        _close(R.act(i, x), R.act(name, x))
    sc, sh, pr = RNG.standard_normal(5), RNG.standard_normal(5), RNG.random(5)
    xx = RNG.standard_normal((2, 3, 4, 5))
    v = F.relu(_t(xx) * _t(sc) + _t(sh))
    _close(R.channel_affine(xx, sc, sh, "relu", pr), torch.where(v > 0, v, v * _t(pr)).numpy())
    v = _t(xx) * _t(sc) + _t(sh)
    _close(R.channel_affine(xx, sc, sh, None, pr), torch.where(v > 0, v, v * _t(pr)).numpy())


def test_binary_matches_torch():
    a, b = RNG.standard_normal((2, 1, 4, 1)), RNG.standard_normal((1, 3, 1, 5))
    fns = {"add": torch.add, "sub": torch.sub, "mul": torch.mul, "div": torch.div, "max": torch.maximum,
           "min": torch.minimum}
    for code, name in enumerate(R.BINARY_OPS):
        if name == "pow":
            continue
        _close(R.binary(name, a, b), fns[name](_t(a), _t(b)).numpy())
        _close(R.binary(code, a, b), R.binary(name, a, b))
    _close(R.binary("pow", np.abs(a) + 0.1, b), torch.pow(_t(np.abs(a) + 0.1), _t(b)).numpy())
    _close(R.binary("pow", a, np.array(2.0)), a * a)
    _close(R.binary("pow", a, np.array(3.0)), a * a * a)
    assert R.BINARY_OPS.index("pow") == 4


def test_softmax_matches_torch():
    x = RNG.standard_normal((2, 3, 65)) * 4
    _close(R.softmax(x), torch.softmax(_t(x), -1).numpy())
    _close(R.softmax(x, 1), torch.softmax(_t(x), 1).numpy())
    _close(R.softmax(x + 300.0), torch.softmax(_t(x + 300.0), -1).numpy())
    x[0, 0, 3:9] = -np.inf
    y = R.softmax(x)
    _close(y, torch.softmax(_t(x), -1).numpy())
    assert np.all(y[0, 0, 3:9] == 0.0)
    _close(R.softmax(np.full((2, 7), 3.25)), np.full((2, 7), 1 / 7))


def test_bmm_matches_torch():
    a, b = RNG.standard_normal((2, 1, 5, 7)), RNG.standard_normal((1, 3, 7, 4))
    c, S = R.bmm(a, b)
    _close(c, torch.matmul(_t(a), _t(b)).numpy())
    _close(S, torch.matmul(_t(a).abs(), _t(b).abs()).numpy())
    c0, S0 = R.bmm(np.zeros((2, 3, 0)), np.zeros((2, 0, 4)))
    assert c0.shape == (2, 3, 4) and not c0.any() and not S0.any()


# ------------------------------------------------------------------ pooling and friends
@pytest.mark.parametrize("k,s,p", [(3, 2, 1), (2, 2, 0), ((3, 2), (2, 1), (1, 0))])
@pytest.mark.parametrize("hw", [(7, 5), (8, 8)])
def test_pool_matches_torch(k, s, p, hw):
    x = RNG.standard_normal((2, hw[0], hw[1], 3)) - 3.0          # mostly negative: padding must not win a max
    y, _ = R.pool2d(x, k, s, p, True)
    _close(R.nchw(y), F.max_pool2d(_t(R.nchw(x)), k, s, p).numpy())
    for cip in (True, False):
        y, S = R.pool2d(x, k, s, p, False, count_include_pad=cip)
        _close(R.nchw(y), F.avg_pool2d(_t(R.nchw(x)), k, s, p, count_include_pad=cip).numpy())
        _close(R.nchw(S), F.avg_pool2d(_t(R.nchw(np.abs(x))), k, s, p, count_include_pad=cip).numpy())


def test_pool_asymmetric_pads():
    x = RNG.standard_normal((1, 5, 6, 2))
    y, _ = R.pool2d(x, 3, 2, (0, 1, 2, 0), True)
    ref = F.max_pool2d(F.pad(_t(R.nchw(x)), (1, 0, 0, 2), value=-np.inf), 3, 2)
    _close(R.nchw(y), ref.numpy())


def test_global_avgpool_upsample_scale_shuffle():
    x = RNG.standard_normal((2, 3, 5, 4))
    y, S = R.global_avgpool(x)
    _close(y, _t(x).mean(dim=(1, 2)).numpy())
    _close(S, _t(x).abs().mean(dim=(1, 2)).numpy())
    add = RNG.standard_normal((2, 9, 15, 4))
    ref = F.interpolate(_t(R.nchw(x)), scale_factor=3, mode="nearest") + _t(R.nchw(add))
    _close(R.nchw(R.upsample_add(x, 3, add)), ref.numpy())
    _close(R.upsample_add(x, 2), R.nhwc(F.interpolate(_t(R.nchw(x)), scale_factor=2, mode="nearest").numpy()))
    s = RNG.random((2, 4))
    _close(R.channel_scale(x, s), (_t(x) * _t(s)[:, None, None, :]).numpy())
    for f, C in ((2, 3), (4, 2)):
        yy = RNG.standard_normal((2, 3, 2, f * f * C))
        # torch's pixel_shuffle wants channel index c*f*f + dy*f + dx
        tin = _t(yy).reshape(2, 3, 2, f, f, C).permute(0, 5, 3, 4, 1, 2).reshape(2, C * f * f, 3, 2)
        ref = F.pixel_shuffle(tin, f).permute(0, 2, 3, 1)
        got = R.depth_to_space(yy, f)
        assert np.array_equal(got, ref.numpy())


@pytest.mark.parametrize("kh,kw,stride,dil,pads", [
    (3, 3, (1, 1), (1, 1), (1, 1, 1, 1)), (3, 3, (2, 2), (1, 1), (0, 0, 1, 1)), (3, 3, (1, 1), (2, 2), (2, 2, 2, 2)),
    (1, 7, (1, 1), (1, 1), (0, 3, 0, 3)), (7, 1, (2, 1), (1, 1), (3, 0, 3, 0)), (3, 5, (3, 3), (1, 1), (1, 2, 1, 2)),
    (2, 2, (1, 2), (1, 1), (0, 0, 0, 0)), (1, 1, (1, 1), (1, 1), (0, 0, 0, 0)), (3, 3, (2, 1), (2, 1), (2, 0, 1, 2))])
def test_depthwise_matches_torch(kh, kw, stride, dil, pads):
    C = 5
    x, w, b = RNG.standard_normal((2, 9, 8, C)), RNG.standard_normal((kh, kw, C)), RNG.standard_normal(C)
    y, S = R.depthwise_conv(x, w, b, stride, dil, pads)
    pt, pl, pb, pr = pads

    def tconv(xx, ww, bb):
        return F.conv2d(F.pad(_t(R.nchw(xx)), (pl, pr, pt, pb)), _t(ww).permute(2, 0, 1).unsqueeze(1).contiguous(),
                        _t(bb), stride, 0, dil, groups=C)

    _close(R.nchw(y), tconv(x, w, b).numpy())
    _close(R.nchw(S), tconv(np.abs(x), np.abs(w), np.abs(b)).numpy())


def test_bf16_round_ties_to_even_and_matches_torch():
    v = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -7, -(1 + 2.0 ** -8), 0.0, 1e-3, 3.14159, 65504.0],
                 np.float32)
    got = R.bf16_round(v)
    assert got[0] == 1.0 and got[1] == 1 + 2.0 ** -6 and got[2] == 1 + 2.0 ** -7 and got[3] == -1.0
    x = RNG.standard_normal(4096).astype(np.float32) * 50
    assert np.array_equal(R.bf16_round(x), torch.from_numpy(x).bfloat16().double().numpy())
