"""Single-node conformance of the ONNX executor's CPU path (the numerics oracle of the GPU path)
against tests/onnx_ref.py and hand-computed vectors: one small case per op whose semantics hang on
an attribute or an optional input."""
import numpy as np
import pytest
import torch

import onnx_ref as R
from lumen_amd.runtime.onnx_graph import OnnxGraph
from lumen_amd.utils import onnx_lite as ox

N = ox.Node
RNG = np.random.default_rng(11)


def run1(op, feeds, init=None, attrs=None, inputs=None, opset=13):
    """Run one node on the CPU path; ``feeds`` name -> array are graph inputs, ``init`` initializers,
    ``inputs`` the node's input list (default: feeds then initializers, in order)."""
    init = init or {}
    names = inputs if inputs is not None else list(feeds) + list(init)
    g = ox.Graph([N(op, names, ["y"], attrs=attrs or {})], init, list(feeds), ["y"])
    out = OnnxGraph(ox.write_model(g, opset=opset)).run({k: torch.from_numpy(np.asarray(v)) for k, v in feeds.items()})
    return out[0].numpy()


def close(got, ref, tol=1e-5):
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(np.abs(got.astype(np.float64) - ref) <= tol * np.maximum(1.0, np.abs(ref))), (got, ref)


def f32(*shape):
    return RNG.standard_normal(shape).astype(np.float32)


def resize_w(vals, wo, ctm):
    x = np.asarray(vals, np.float32).reshape(1, 1, 1, -1)
    sizes = np.array([1, 1, 1, wo], np.int64)
    return run1("Resize", {"x": x}, {"sizes": sizes}, {"mode": "linear", "coordinate_transformation_mode": ctm},
                inputs=["x", "", "", "sizes"]).reshape(-1)


# ------------------------------------------------------------------ the six known-wrong rows
def test_resize_linear_asymmetric():
    close(resize_w([0, 1, 2, 3], 8, "asymmetric"), [0, .5, 1, 1.5, 2, 2.5, 3, 3])


def test_resize_linear_pytorch_half_pixel_length_one():
    close(resize_w([0, 1, 2, 3], 1, "pytorch_half_pixel"), [0.0])


def test_max_min_variadic():
    a, b, c = f32(2, 3), f32(2, 3), f32(1, 3)
    feeds = {"a": a, "b": b, "c": c}
    close(run1("Max", feeds), np.maximum(np.maximum(a, b), c))
    close(run1("Min", feeds), np.minimum(np.minimum(a, b), c))
    close(run1("Max", {"a": a}), a)


def test_reducemean_axes_input():
    x = f32(2, 3, 4)
    got = run1("ReduceMean", {"x": x}, {"axes": np.array([1], np.int64)}, {"keepdims": 1}, opset=18)
    close(got, x.astype(np.float64).mean(axis=1, keepdims=True))
    got = run1("ReduceMean", {"x": x}, {"axes": np.array([-1, 0], np.int64)}, {"keepdims": 0}, opset=18)
    close(got, x.astype(np.float64).mean(axis=(0, 2)))


def test_gather_negative_index():
    x = f32(4, 3)
    close(run1("Gather", {"x": x}, {"i": np.array(-1, np.int64)}, {"axis": 0}), x[-1])
    close(run1("Gather", {"x": x}, {"i": np.array([[0, -1], [-3, 2]], np.int64)}, {"axis": 1}),
          x[:, np.array([[0, 2], [0, 2]])])


def test_slice_negative_step():
    x = f32(5, 4)
    i64 = lambda *v: np.array(v, np.int64)      # noqa: E731
    init = {"st": i64(-1), "en": i64(-(2 ** 63)), "ax": i64(0), "sp": i64(-1)}
    close(run1("Slice", {"x": x}, init), x[::-1])
    init = {"st": i64(3, 1), "en": i64(0, 4), "ax": i64(0, 1), "sp": i64(-2, 2)}
    close(run1("Slice", {"x": x}, init), x[3:0:-2, 1:4:2])
    init = {"st": i64(100), "en": i64(-3), "ax": i64(1), "sp": i64(-1)}      # start clamps to dim - 1
    close(run1("Slice", {"x": x}, init), x[:, 3:1:-1])


# ------------------------------------------------------------------ the other resize modes
@pytest.mark.parametrize("ctm", R.RESIZE_MODES)
@pytest.mark.parametrize("src,dst", [((3, 5), (7, 8)), ((7, 9), (3, 4)), ((4, 6), (1, 1)), ((1, 1), (4, 4)),
                                     ((2, 3), (1, 7))])
def test_resize_linear_modes(ctm, src, dst):
    x = f32(2, 3, *src)
    got = run1("Resize", {"x": x}, {"sizes": np.array([2, 3, *dst], np.int64)},
               {"mode": "linear", "coordinate_transformation_mode": ctm}, inputs=["x", "", "", "sizes"])
    ref, _ = R.resize_bilinear_nhwc(R.nhwc(x), dst[0], dst[1], ctm)
    close(got, R.nchw(ref))


def test_resize_linear_scales_input_and_unknown_mode():
    x = f32(1, 2, 3, 4)
    got = run1("Resize", {"x": x}, {"roi": np.zeros(0, np.float32), "sc": np.array([1, 1, 2, 2], np.float32)},
               {"mode": "linear", "coordinate_transformation_mode": "asymmetric"})
    close(got, R.nchw(R.resize_bilinear_nhwc(R.nhwc(x), 6, 8, "asymmetric")[0]))
    with pytest.raises(NotImplementedError):
        run1("Resize", {"x": x}, {"roi": np.zeros(0, np.float32), "sc": np.array([1, 1, 2, 2], np.float32)},
             {"mode": "linear", "coordinate_transformation_mode": "tf_crop_and_resize"})


# ------------------------------------------------------------------ attribute-dependent ops
def test_averagepool_count_include_pad():
    x = f32(1, 2, 5, 5)
    at = {"kernel_shape": [3, 3], "strides": [2, 2], "pads": [1, 1, 1, 1]}
    for cip in (0, 1):
        ref, _ = R.pool2d(R.nhwc(x), 3, 2, 1, False, count_include_pad=bool(cip))
        close(run1("AveragePool", {"x": x}, attrs={**at, "count_include_pad": cip}), R.nchw(ref))
    ref, _ = R.pool2d(R.nhwc(x), 3, 2, 1, False, count_include_pad=False)
    close(run1("AveragePool", {"x": x}, attrs=at), R.nchw(ref))            # the ONNX default is 0
    corner = x[0, 0, :2, :2].astype(np.float64).sum()
    got = run1("AveragePool", {"x": x}, attrs={**at, "count_include_pad": 1})
    close(got[0, 0, 0, 0], corner / 9)
    close(run1("AveragePool", {"x": x}, attrs=at)[0, 0, 0, 0], corner / 4)


def test_averagepool_ceil_mode():
    x = np.arange(9, dtype=np.float32).reshape(1, 1, 3, 3)
    at = {"kernel_shape": [2, 2], "strides": [2, 2]}
    close(run1("AveragePool", {"x": x}, attrs=at), [[[[2.0]]]])
    # ceil_mode keeps the partial windows; they average the pixels they hold
    close(run1("AveragePool", {"x": x}, attrs={**at, "ceil_mode": 1}), [[[[2.0, 3.5], [6.5, 8.0]]]])


def test_averagepool_asymmetric_pads_exclude_padding():
    x = f32(1, 2, 4, 5)
    got = run1("AveragePool", {"x": x}, attrs={"kernel_shape": [2, 2], "strides": [2, 2], "pads": [0, 0, 0, 1]})
    ref, _ = R.pool2d(R.nhwc(x), 2, 2, (0, 0, 0, 1), False, count_include_pad=False)
    close(got, R.nchw(ref))
    got = run1("AveragePool", {"x": x}, attrs={"kernel_shape": [2, 2], "strides": [2, 2], "pads": [0, 0, 0, 1],
                                               "count_include_pad": 1})
    ref, _ = R.pool2d(R.nhwc(x), 2, 2, (0, 0, 0, 1), False, count_include_pad=True)
    close(got, R.nchw(ref))


def test_maxpool_asymmetric_pads():
    x = f32(1, 2, 5, 6) - 3.0           # negative values: padding must never win
    got = run1("MaxPool", {"x": x}, attrs={"kernel_shape": [3, 3], "strides": [2, 2], "pads": [0, 1, 2, 0]})
    ref, _ = R.pool2d(R.nhwc(x), 3, 2, (0, 1, 2, 0), True)
    close(got, R.nchw(ref))


def test_clip_single_bound():
    x = f32(3, 7) * 3
    hi, lo = np.array(0.5, np.float32), np.array(-0.25, np.float32)
    close(run1("Clip", {"x": x}, {"hi": hi}, inputs=["x", "", "hi"]), np.minimum(x, 0.5))
    close(run1("Clip", {"x": x}, {"lo": lo}, inputs=["x", "lo"]), np.maximum(x, -0.25))
    close(run1("Clip", {"x": x}, {"lo": lo, "hi": hi}), np.clip(x, -0.25, 0.5))
    close(run1("Clip", {"x": x}, attrs={"max": 0.5}, opset=6), np.minimum(x, 0.5))


def test_squeeze_unsqueeze_negative_axes():
    x = f32(3, 1, 4, 1)
    i64 = lambda *v: np.array(v, np.int64)      # noqa: E731
    assert run1("Squeeze", {"x": x}, {"ax": i64(-1)}).shape == (3, 1, 4)
    assert run1("Squeeze", {"x": x}, {"ax": i64(-3, -1)}).shape == (3, 4)
    assert run1("Squeeze", {"x": x}).shape == (3, 4)
    y = f32(3, 4)
    assert run1("Unsqueeze", {"x": y}, {"ax": i64(-1)}).shape == (3, 4, 1)
    assert run1("Unsqueeze", {"x": y}, {"ax": i64(-1, -2)}).shape == (3, 4, 1, 1)     # axes index the OUTPUT rank
    assert run1("Unsqueeze", {"x": y}, {"ax": i64(-3, 0)}).shape == (1, 1, 3, 4)
    assert run1("Unsqueeze", {"x": y}, {"ax": i64(0, -1)}).shape == (1, 3, 4, 1)
    assert run1("Unsqueeze", {"x": y}, attrs={"axes": [1]}, opset=11).shape == (3, 1, 4)
    close(run1("Unsqueeze", {"x": y}, {"ax": i64(-2)}), y[:, None, :])


def test_flatten_axes():
    x = f32(2, 3, 4)
    close(run1("Flatten", {"x": x}, attrs={"axis": 0}), x.reshape(1, 24))
    close(run1("Flatten", {"x": x}, attrs={"axis": -1}), x.reshape(6, 4))
    close(run1("Flatten", {"x": x}), x.reshape(2, 12))
    close(run1("Flatten", {"x": x}, attrs={"axis": 2}), x.reshape(6, 4))


def test_reshape_zero_and_minus_one():
    x = f32(2, 3, 4)
    close(run1("Reshape", {"x": x}, {"s": np.array([0, -1], np.int64)}), x.reshape(2, 12))
    close(run1("Reshape", {"x": x}, {"s": np.array([-1, 0, 2, 2], np.int64)}), x.reshape(2, 3, 2, 2))
    close(run1("Reshape", {"x": x}, {"s": np.array([4, -1], np.int64)}), x.reshape(4, 6))


def test_argmax_keepdims():
    x = f32(3, 5, 2)
    for ax in (0, 1, -1):
        got = run1("ArgMax", {"x": x}, attrs={"axis": ax, "keepdims": 1})
        assert np.array_equal(got, np.expand_dims(x.argmax(axis=ax), ax))
        got = run1("ArgMax", {"x": x}, attrs={"axis": ax, "keepdims": 0})
        assert np.array_equal(got, x.argmax(axis=ax))
    assert run1("ArgMax", {"x": x}).shape == (1, 5, 2)          # defaults: axis 0, keepdims 1


def test_softmax_non_last_axis():
    x = f32(2, 3, 4, 5) * 3
    for ax in (1, -2, 0, 3):
        close(run1("Softmax", {"x": x}, attrs={"axis": ax}), R.softmax(x, ax))
    close(run1("Softmax", {"x": x}), R.softmax(x, -1))


def test_layernormalization_last_axis():
    x, g, b = f32(2, 5, 16) * 2 + 1, f32(16), f32(16)
    x64 = x.astype(np.float64)
    mu, var = x64.mean(-1, keepdims=True), x64.var(-1, keepdims=True)
    ref = (x64 - mu) / np.sqrt(var + 1e-3) * g + b
    close(run1("LayerNormalization", {"x": x}, {"g": g, "b": b}, {"axis": -1, "epsilon": 1e-3}), ref, 1e-4)
    ref = (x64 - mu) / np.sqrt(var + 1e-5) * g
    close(run1("LayerNormalization", {"x": x}, {"g": g}, opset=17), ref, 1e-4)


def test_hardsigmoid_leakyrelu_parameters():
    x = f32(4, 9) * 4
    close(run1("HardSigmoid", {"x": x}, attrs={"alpha": 0.25, "beta": 0.375}), R.unary("hardsigmoid", x, 0.25, 0.375))
    close(run1("HardSigmoid", {"x": x}), R.unary("hardsigmoid", x, 0.2, 0.5))
    close(run1("LeakyRelu", {"x": x}, attrs={"alpha": 0.125}), R.unary("leaky", x, 0.125))
    close(run1("LeakyRelu", {"x": x}), R.unary("leaky", x, 0.01))


def test_depthwise_conv_asymmetric_pads_and_prelu():
    x, w, b = f32(2, 4, 7, 6), f32(8, 1, 3, 3), f32(8)
    sl = (RNG.random(8) * 0.5).astype(np.float32)
    g = ox.Graph([N("Conv", ["x", "w", "b"], ["c"], attrs={"kernel_shape": [3, 3], "pads": [0, 0, 1, 1],
                                                          "strides": [2, 2], "group": 4}),
                  N("PRelu", ["c", "sl"], ["y"])], {"w": w, "b": b, "sl": sl}, ["x"], ["y"])
    got = OnnxGraph(ox.write_model(g)).run({"x": torch.from_numpy(x)})[0].numpy()
    xr = np.repeat(R.nhwc(x), 2, axis=3)                # channel multiplier 2: output c reads input c // 2
    ref, _ = R.depthwise_conv(xr, w.reshape(8, 3, 3).transpose(1, 2, 0), b, 2, 1, (0, 0, 1, 1))
    ref = np.where(ref > 0, ref, ref * sl)
    close(got, R.nchw(ref), 1e-4)
