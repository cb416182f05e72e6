"""The step buffer of the decode graphs (runtime/decode_graphs.py): the table-driven layouts equal
the hand-written ones they replaced (tests/golden/step_layouts.json, recorded from those), and
staging pads what a step does not cover.  Plain CPU tensors: no GPU, no pinned memory."""
import json
import os

import numpy as np
import pytest
import torch

from lumen_amd.runtime.decode_graphs import FIELDS, MODES, ROW, SEQ, is_verify, stage, step_layout, step_views

DECODE_SHAPES = [(1, 8, 1), (3, 8, 1), (4, 32, 1), (128, 128, 1)]
VERIFY_SHAPES = [(1, 8, 4), (3, 8, 4), (8, 32, 4), (4, 8, 8), (16, 128, 2)]
CASES = [(m, s) for m in MODES for s in (VERIFY_SHAPES if is_verify(m) else DECODE_SHAPES)]
PADS = {"slots": -1, "ids": 0, "pos": 0, "ctx": 1, "n_rows": 1, "bt": 0, "u": 0.0, "top_p": 1.0, "inv_t": 1.0,
        "penalty": 1.0, "greedy": 1, "seen_slot": -1, "g_slot": -1, "g_in": -1}

with open(os.path.join(os.path.dirname(__file__), "golden", "step_layouts.json")) as f:
    GOLDEN = json.load(f)


def test_the_six_modes():
    assert sorted(MODES) == ["greedy", "guided", "sample", "verify", "verify_guided", "verify_sample"]
    assert len(GOLDEN) == len(CASES)
    assert {f.name: f.pad for fs in FIELDS.values() for f in fs} == PADS


@pytest.mark.parametrize("mode,shape", CASES)
def test_layout_equals_the_recorded_one(mode, shape):
    Bp, W, T = shape
    lay, total = step_layout(mode, Bp, W, T)
    want = GOLDEN[f"{mode}:{Bp}:{W}:{T}"]
    assert total == want["bytes"]
    assert {k: list(v) for k, v in lay.items()} == want["fields"]
    assert list(lay) == [f.name for f in FIELDS[mode]]


def test_anchor_values():
    def at(mode, Bp, W, T=1):
        lay, total = step_layout(mode, Bp, W, T)
        return total, {k: o for k, (o, _n) in lay.items()}

    assert at("greedy", 4, 32)[0] == 576
    total, off = at("guided", 3, 8)
    assert (total, off["u"], off["g_slot"], off["g_in"]) == (272, 144, 240, 252)
    total, off = at("verify", 3, 8, 4)
    assert (total, off["n_rows"]) == (368, 252)
    total, off = at("verify_sample", 8, 32, 4)
    assert (total, off["u"]) == (2176, 1728)
    total, off = at("verify_guided", 3, 8, 4)
    assert (total, off["u"], off["g_in"]) == (592, 368, 544)
    assert at("verify_guided", 4, 8, 8)[0] == 1280


@pytest.mark.parametrize("mode,shape", CASES)
def test_layout_structure(mode, shape):
    Bp, W, T = shape
    lay, total = step_layout(mode, Bp, W, T)
    assert total % 16 == 0
    end = 0
    for f in FIELDS[mode]:                      # in buffer order: no overlap, natural alignment
        o, n = lay[f.name]
        assert o >= end and o % f.dtype.itemsize == 0, f.name
        assert n == {ROW: Bp * T, SEQ: Bp}.get(f.extent, Bp * W), f.name
        end = o + n * f.dtype.itemsize
    assert end <= total
    for group in MODES[mode]:
        assert lay[group[0].name][0] % 16 == 0, group[0].name


def _values(mode, B, T, width, seed):
    """recognisable values, none equal to its field's pad, in each field's dtype"""
    rng = np.random.default_rng(seed)
    out = {}
    for f in FIELDS[mode]:
        dt = torch.empty(0, dtype=f.dtype).numpy().dtype
        n = {ROW: B * T, SEQ: B}.get(f.extent)
        shape = (B, width) if n is None else (n,)
        if dt.kind == "f":
            out[f.name] = (rng.integers(2, 100, shape) / 128.0 + 2).astype(dt)
        else:
            out[f.name] = rng.integers(100, 10000, shape).astype(dt)
    return out


@pytest.mark.parametrize("mode", list(MODES))
def test_staging_pads_what_a_smaller_step_leaves(mode):
    Bp, W, T = 4, 8, 4 if is_verify(mode) else 1
    buf = torch.zeros(step_layout(mode, Bp, W, T)[1], dtype=torch.uint8)
    views = step_views(buf, mode, Bp, W, T, numpy=True)
    first = _values(mode, 3, T, 5, seed=1)
    stage(views, mode, first)
    for f in FIELDS[mode]:                      # B = 3, table 5 wide: the leading entries, the pad elsewhere
        a, v = views[f.name], first[f.name]
        if f.name == "bt":
            assert np.array_equal(a[:3, :5], v) and (a[:3, 5:] == 0).all() and (a[3:] == 0).all()
        else:
            assert np.array_equal(a[:len(v)], v) and (a[len(v):] == f.pad).all(), f.name
    second = _values(mode, 1, T, 11, seed=2)
    stage(views, mode, second)
    again = step_views(buf, mode, Bp, W, T)    # read back through fresh tensor views of the same bytes
    for f in FIELDS[mode]:
        a, v = again[f.name], second[f.name]
        assert a.dtype == f.dtype
        a = a.numpy()
        assert a.dtype == v.dtype
        if f.name == "bt":
            assert a.shape == (Bp, W)
            assert np.array_equal(a[0], v[0, :W])           # columns beyond W are dropped
            assert (a[1:] == PADS["bt"]).all()
        else:
            n = len(v)
            assert n == (T if f.extent is ROW else 1)
            assert np.array_equal(a[:n], v), f.name
            assert a.shape == (Bp * T if f.extent is ROW else Bp,)
            assert (a[n:] == PADS[f.name]).all(), f.name    # nothing of the first step survives


@pytest.mark.parametrize("mode", list(MODES))
def test_staging_a_missing_field_raises(mode):
    Bp, W, T = 4, 8, 4 if is_verify(mode) else 1
    buf = torch.zeros(step_layout(mode, Bp, W, T)[1], dtype=torch.uint8)
    views = step_views(buf, mode, Bp, W, T, numpy=True)
    vals = _values(mode, 2, T, 8, seed=3)
    for f in FIELDS[mode]:
        with pytest.raises(KeyError, match=f.name):
            stage(views, mode, {k: v for k, v in vals.items() if k != f.name})


def test_views_refuse_a_buffer_of_another_size():
    with pytest.raises(ValueError):
        step_views(torch.zeros(560, dtype=torch.uint8), "greedy", 4, 32)
