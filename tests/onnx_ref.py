"""Float64 numpy references for the ONNX node kernels (csrc/onnx_ops.hip) and the NHWC helper
kernels (csrc/conv.hip), written from the ONNX operator definitions.

Nothing here imports lumen_amd.  Every function takes the values the kernel sees (bf16 inputs
already rounded, widened to float64) and works in float64 throughout.  Reductions and blends also
return ``S``, the sum of the absolute contributions per output element (``sum |a_i * b_i|``), which
is what a rounding-error bound of the f32 / bf16 kernels scales with.

Activations are NHWC ``[N, H, W, C]`` as in the kernels; :func:`nchw` / :func:`nhwc` convert for
the ONNX-level (NCHW) node tests.  tests/test_onnx_ref_cpu.py checks this module against torch's
float64 CPU ops and hand-computed vectors.
"""
from __future__ import annotations

import math

import numpy as np

BINARY_OPS = ("add", "sub", "mul", "div", "pow", "max", "min")                   # ew_binary codes 0..6
UNARY_OPS = ("relu", "sigmoid", "tanh", "exp", "log", "sqrt", "neg", "abs", "reciprocal", "hardswish",
             "hardsigmoid", "leaky", "clip", "floor", "ceil", "erf", "identity")  # ew_unary codes 0..16
RESIZE_MODES = ("half_pixel", "align_corners", "asymmetric", "pytorch_half_pixel")  # kernel modes 0..3
ACTS = ("none", "gelu", "quick_gelu", "relu", "silu", "gelu_tanh", "hardswish", "sigmoid", "leaky",
        "hardsigmoid")                                                             # common.h Act 0..9

_erf = np.vectorize(math.erf, otypes=[np.float64])


def f64(x) -> np.ndarray:
    """torch tensor / array -> float64 numpy array (exact for f32 and bf16 values)."""
    if hasattr(x, "detach"):
        x = x.detach().cpu().double().numpy()
    return np.asarray(x, dtype=np.float64)


def bf16_round(x) -> np.ndarray:
    """Round float32 values to bfloat16 (nearest, ties to even); result widened to float64."""
    f = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    u = f.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32).astype(np.float64).reshape(f.shape)


def nchw(x):
    return np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2)))


def nhwc(x):
    return np.ascontiguousarray(np.transpose(x, (0, 2, 3, 1)))


# ------------------------------------------------------------------ elementwise
def binary(op, a, b) -> np.ndarray:
    """Numpy-broadcast binary op; ``op`` a code 0..6 or a name of BINARY_OPS."""
    name = BINARY_OPS[op] if isinstance(op, int) else op
    a, b = f64(a), f64(b)
    with np.errstate(all="ignore"):
        return {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide, "pow": np.power,
                "max": np.maximum, "min": np.minimum}[name](a, b)


def unary(op, x, p0: float = 0.0, p1: float = 0.0) -> np.ndarray:
    """``op`` a code 0..16 or a name of UNARY_OPS; p0 / p1: hardsigmoid (alpha, beta), leaky
    (alpha), clip (lo, hi)."""
    name = UNARY_OPS[op] if isinstance(op, int) else op
    x = f64(x)
    with np.errstate(all="ignore"):
        if name == "relu":
            return np.maximum(x, 0.0)
        if name == "sigmoid":
            return 1.0 / (1.0 + np.exp(-x))
        if name == "tanh":
            return np.tanh(x)
        if name == "exp":
            return np.exp(x)
        if name == "log":
            return np.log(x)
        if name == "sqrt":
            return np.sqrt(x)
        if name == "neg":
            return -x
        if name == "abs":
            return np.abs(x)
        if name == "reciprocal":
            return 1.0 / x
        if name == "hardswish":
            return x * np.clip(x + 3.0, 0.0, 6.0) / 6.0
        if name == "hardsigmoid":
            return np.clip(x * p0 + p1, 0.0, 1.0)
        if name == "leaky":
            return np.where(x > 0.0, x, x * p0)
        if name == "clip":
            return np.minimum(np.maximum(x, p0), p1)
        if name == "floor":
            return np.floor(x)
        if name == "ceil":
            return np.ceil(x)
        if name == "erf":
            return _erf(x)
        if name == "identity":
            return x.copy()
    raise ValueError(name)


def act(name_or_id, x) -> np.ndarray:
    """The fused activations of the conv / affine epilogues (common.h Act 0..9)."""
    name = ACTS[name_or_id] if isinstance(name_or_id, int) else (name_or_id or "none")
    x = f64(x)
    with np.errstate(all="ignore"):
        if name == "none":
            return x.copy()
        if name == "gelu":
            return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))
        if name == "quick_gelu":
            return x / (1.0 + np.exp(-1.702 * x))
        if name == "relu":
            return np.maximum(x, 0.0)
        if name == "silu":
            return x / (1.0 + np.exp(-x))
        if name == "gelu_tanh":
            return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
        if name == "hardswish":
            return x * np.clip(x + 3.0, 0.0, 6.0) / 6.0
        if name == "sigmoid":
            return 1.0 / (1.0 + np.exp(-x))
        if name == "leaky":
            return np.where(x > 0.0, x, 0.1 * x)
        if name == "hardsigmoid":
            return np.clip(x / 6.0 + 0.5, 0.0, 1.0)
    raise ValueError(name)


def softmax(x, axis: int = -1) -> np.ndarray:
    x = f64(x)
    with np.errstate(all="ignore"):
        e = np.exp(x - np.max(x, axis=axis, keepdims=True))
    return e / np.sum(e, axis=axis, keepdims=True)


# ------------------------------------------------------------------ matmul
def bmm(a, b):
    """Batched (numpy-broadcast) matmul -> (c, S) with S = sum_k |a_mk * b_kn|."""
    a, b = f64(a), f64(b)
    return np.matmul(a, b), np.matmul(np.abs(a), np.abs(b))


# ------------------------------------------------------------------ resize
def resize_coords(osz: int, isz: int, mode) -> np.ndarray:
    """Source coordinate of every output index along one axis (ONNX Resize
    coordinate_transformation_mode, scale = osz / isz), before clamping."""
    name = RESIZE_MODES[mode] if isinstance(mode, int) else mode
    o = np.arange(osz, dtype=np.float64)
    s = isz / osz
    if name == "half_pixel":
        return (o + 0.5) * s - 0.5
    if name == "align_corners":
        return o * (isz - 1) / (osz - 1) if osz > 1 else np.zeros(osz)
    if name == "asymmetric":
        return o * s
    if name == "pytorch_half_pixel":
        return (o + 0.5) * s - 0.5 if osz > 1 else np.zeros(osz)
    raise ValueError(name)


def _taps(osz, isz, mode):
    f = np.clip(resize_coords(osz, isz, mode), 0.0, isz - 1)
    i0 = np.floor(f).astype(np.int64)
    i1 = np.minimum(i0 + 1, isz - 1)
    return i0, i1, f - i0


def resize_bilinear_nhwc(x, Ho: int, Wo: int, mode):
    """NHWC bilinear resize: coordinate map, clamp to [0, in - 1], 4-tap blend -> (y, S) with
    S = sum |w_i * p_i| over the four taps."""
    x = f64(x)
    H, W = x.shape[1], x.shape[2]
    y0, y1, wy = _taps(Ho, H, mode)
    x0, x1, wx = _taps(Wo, W, mode)
    wy = wy[None, :, None, None]
    wx = wx[None, None, :, None]

    def blend(v):
        top = v[:, y0][:, :, x0] * (1 - wx) + v[:, y0][:, :, x1] * wx
        bot = v[:, y1][:, :, x0] * (1 - wx) + v[:, y1][:, :, x1] * wx
        return top * (1 - wy) + bot * wy

    return blend(x), blend(np.abs(x))


# ------------------------------------------------------------------ pooling
def _pair(v):
    return (int(v), int(v)) if isinstance(v, (int, np.integer)) else (int(v[0]), int(v[1]))


def _pads4(p):
    if isinstance(p, (int, np.integer)):
        return (int(p),) * 4
    p = tuple(int(q) for q in p)
    return p if len(p) == 4 else (p[0], p[1], p[0], p[1])


def pool2d(x, kernel, stride, padding=0, is_max: bool = True, count_include_pad: bool = True):
    """NHWC max / average pooling, floor output size; ``padding`` int, (ph, pw) or (top, left,
    bottom, right) -> (y, S).  S is |y| for max pooling and sum |x_i| / divisor for average."""
    x = f64(x)
    N, H, W, C = x.shape
    (kh, kw), (sh, sw) = _pair(kernel), _pair(stride)
    pt, pl, pb, pr = _pads4(padding)
    Ho, Wo = (H + pt + pb - kh) // sh + 1, (W + pl + pr - kw) // sw + 1
    fill = -np.inf if is_max else 0.0
    xp = np.full((N, H + pt + pb, W + pl + pr, C), fill)
    xp[:, pt:pt + H, pl:pl + W] = x
    inside = np.zeros((1, H + pt + pb, W + pl + pr, 1))
    inside[:, pt:pt + H, pl:pl + W] = 1.0
    y = np.full((N, Ho, Wo, C), fill)
    S = np.zeros((N, Ho, Wo, C))
    cnt = np.zeros((1, Ho, Wo, 1))
    for ky in range(kh):
        for kx in range(kw):
            win = (slice(None), slice(ky, ky + (Ho - 1) * sh + 1, sh), slice(kx, kx + (Wo - 1) * sw + 1, sw))
            if is_max:
                y = np.maximum(y, xp[win])
            else:
                y = y + xp[win]
                S = S + np.abs(xp[win])
                cnt = cnt + inside[win]
    if is_max:
        return y, np.abs(y)
    div = float(kh * kw) if count_include_pad else cnt
    return y / div, S / div


def global_avgpool(x):
    """NHWC -> [N, C] mean over H, W -> (y, S = mean |x|)."""
    x = f64(x)
    return x.mean(axis=(1, 2)), np.abs(x).mean(axis=(1, 2))


def upsample_add(x, factor: int, add=None) -> np.ndarray:
    """Nearest upsample by an integer factor (out[h, w] = x[h // f, w // f]) plus ``add``."""
    y = np.repeat(np.repeat(f64(x), factor, axis=1), factor, axis=2)
    return y if add is None else y + f64(add)


def channel_scale(x, s) -> np.ndarray:
    """x[n, h, w, c] * s[n, c]."""
    return f64(x) * f64(s)[:, None, None, :]


def channel_affine(x, scale, shift, act_name=None, prelu=None) -> np.ndarray:
    """prelu(act(x * scale[c] + shift[c]))."""
    y = act(act_name, f64(x) * f64(scale) + f64(shift))
    if prelu is not None:
        y = np.where(y > 0.0, y, y * f64(prelu))
    return y


def depth_to_space(y, f: int) -> np.ndarray:
    """[N, H, W, f*f*C] with channel index (dy*f + dx)*C + c -> [N, H*f, W*f, C]."""
    y = f64(y)
    N, H, W, CC = y.shape
    C = CC // (f * f)
    return y.reshape(N, H, W, f, f, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, H * f, W * f, C)


# ------------------------------------------------------------------ depthwise conv
def depthwise_conv(x, w, bias=None, stride=1, dilation=1, pads=0):
    """NHWC depthwise convolution, w [KH, KW, C]; stride / dilation per axis, pads int, (ph, pw) or
    (top, left, bottom, right) -> (y, S) with S = sum |w_i * x_i| + |bias|."""
    x, w = f64(x), f64(w)
    N, H, W, C = x.shape
    KH, KW, _ = w.shape
    (sh, sw), (dh, dw) = _pair(stride), _pair(dilation)
    pt, pl, pb, pr = _pads4(pads)
    Ho = (H + pt + pb - dh * (KH - 1) - 1) // sh + 1
    Wo = (W + pl + pr - dw * (KW - 1) - 1) // sw + 1
    xp = np.zeros((N, H + pt + pb, W + pl + pr, C))
    xp[:, pt:pt + H, pl:pl + W] = x
    y = np.zeros((N, Ho, Wo, C))
    S = np.zeros((N, Ho, Wo, C))
    for ky in range(KH):
        for kx in range(KW):
            win = xp[:, ky * dh: ky * dh + (Ho - 1) * sh + 1: sh, kx * dw: kx * dw + (Wo - 1) * sw + 1: sw]
            y = y + win * w[ky, kx]
            S = S + np.abs(win * w[ky, kx])
    if bias is not None:
        y = y + f64(bias)
        S = S + np.abs(f64(bias))
    return y, S


# ------------------------------------------------------------------ comparison helpers
EPS_BF16, EPS_F32 = 2.0 ** -8, 2.0 ** -23
F32_MAX = float(np.finfo(np.float32).max)
BF16_OVERFLOW = 2.0 ** 128 * (1 - 2.0 ** -9)      # f32 values from here up round to inf in bf16


def bound_bf16(S) -> np.ndarray:
    """bf16 output: one bf16 rounding (2^-9) plus f32 arithmetic, on a magnitude S."""
    with np.errstate(invalid="ignore"):
        return EPS_BF16 * np.asarray(S, np.float64) + 1e-6


def bound_f32(S, K: int = 1) -> np.ndarray:
    """f32 output of exact-arithmetic ops: K the reduction length (1 for element-wise ops)."""
    with np.errstate(invalid="ignore"):
        return (K + 2) * EPS_F32 * np.asarray(S, np.float64)


def out_range(ref, bf16: bool) -> np.ndarray:
    """The float64 reference as the output format can hold it: overflow becomes +-inf."""
    lim = BF16_OVERFLOW if bf16 else F32_MAX
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(ref) > lim, np.sign(ref) * np.inf, ref)


def compare(got, ref, bound, what: str = "") -> None:
    """Every element: non-finite reference values must match exactly, the rest within ``bound``."""
    got = f64(got)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin]), (what, got[~fin], ref[~fin])
    err = np.abs(got[fin] - ref[fin])
    ok = err <= bound[fin]
    if not ok.all():
        i = int(np.argmax(np.where(ok, 0.0, np.where(np.isnan(err), np.inf, err))))
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} elements out of bound; worst got "
                             f"{got[fin][i]!r} ref {ref[fin][i]!r} err {err[i]:.3e} bound {bound[fin][i]:.3e}")
