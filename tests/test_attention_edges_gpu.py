"""Dense attention (csrc/attention.hip: the streaming attn_fwd_kernel and the K/V-resident
attn_res_kernel) at its edges, every output element checked against tests/attention_ref.py:

* exact masks -- the visibility probe (q = 0, one-hot V) at key lengths 0, 1, around 16 and around the
  64-key chunk boundaries, causal with Sk != Sq and Sq > Sk, Sq = 1;
* the online-softmax rescale -- ladder inputs whose running max moves by less than, exactly and more
  than the lazy threshold of 8 log2 units inside one wave, rising and falling;
* peaked random inputs in the packed-QKV and LLM layouts with GQA, per-element bound 3 * 2^-8 * (P @ |V|);
* out= views inside a sentinel-filled buffer -- nothing outside the view may change;
* attention_mx with a bf16 out on the same probes and ladders.

tests/test_attention_ref_cpu.py proves on the CPU that an emulation of the kernels passes every case
here and that planted bugs (no rescale, masks off by one, wrong GQA head, a key counted twice) fail.
"""
import pytest
import torch

import attention_ref as A
from lumen_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TUNE_ATTN_CLEAN_CHUNKS = 1          # csrc/tuning.h


def _dev(t):
    return None if t is None else t.to(DEV)


def _expect_path(B, H, Sq, Sk, D, want_resident, waves=None):
    """Every table says which kernel it means to hit (the dispatch rule of attn_fwd, mirrored in
    attention_ref.resident / resident_waves), so a table cannot drift onto the other one."""
    assert A.resident(B, H, Sq, Sk, D) == want_resident, (B, H, Sq, Sk, D)
    if waves is not None:
        assert A.resident_waves(Sq, D) == waves, (Sq, D)


def _run_probe(p, causal, what):
    got = ops.attention(_dev(p["q"]), _dev(p["k"]), _dev(p["v"]), causal=causal, kv_len=_dev(p["kv_len"]))
    A.check_visibility(got, p, causal, what)


# --------------------------------------------------------------------------- 1. exact masks, streaming
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [32, 64, 128])
def test_visibility_streaming(D, causal):
    H, Hkv = A.VIS_STREAM_HEADS
    for Sq, Sk in A.vis_stream_shapes():
        for kvs in (A.kv_len_values(Sk), None):
            p = A.visibility_probe(Sq, Sk, H, Hkv, D, kvs)
            _expect_path(p["q"].shape[0], H, Sq, Sk, D, False)
            _run_probe(p, causal, f"Sq={Sq} Sk={Sk} kv_len={'set' if kvs else None}")


# --------------------------------------------------------------------------- 2. exact masks, resident
@pytest.mark.parametrize("Hkv", [16, 4])
@pytest.mark.parametrize("D,Sq,Sk,causal,clean", A.VIS_RESIDENT)
def test_visibility_resident(D, Sq, Sk, causal, clean, Hkv):
    B, H = 64, 16
    _expect_path(B, H, Sq, Sk, D, True, 8 if Sq == 150 else 4)
    kvs = A.kv_len_values(Sk)
    pairs = -(-Sk // D) * len(kvs)            # (probe pass, kv_len) pairs, 64 per launch (the last one wraps)
    hip = ops.hip_ops()
    base = hip.set_tuning(TUNE_ATTN_CLEAN_CHUNKS, clean)
    try:
        for start in range(0, pairs, B):
            _run_probe(A.visibility_probe(Sq, Sk, H, Hkv, D, kvs, B=B, start=start), causal, f"pairs from {start}")
        if clean:
            _run_probe(A.visibility_probe(Sq, Sk, H, Hkv, D, None, B=B), causal, "kv_len=None")
    finally:
        hip.set_tuning(TUNE_ATTN_CLEAN_CHUNKS, base)


# --------------------------------------------------------------------------- 3. the rescale
_worst = {}


def _note(path, ratio):
    _worst[path] = max(_worst.get(path, 0.0), ratio)
    print(f"check_elements worst ratio so far, {path}: {_worst[path]:.3f}")


def _run_ladder(case, causal, want_resident, attn):
    B, H, Hkv, Sq, Sk, D, steps, kvs = case
    _expect_path(B, H, Sq, Sk, D, want_resident)
    scale = A.default_scale(D)
    q, k, v = A.ladder(1, Sq, Sk, H, Hkv, D, scale, steps)
    nb = len(kvs) if kvs else 1                                     # the reference: once per distinct entry
    kl = None if kvs is None else torch.tensor(kvs, dtype=torch.int32)
    o, w = A.ref64(*(t.expand(nb, *t.shape[1:]) for t in (q, k, v)), scale, causal, kl)
    idx = torch.arange(B) % nb
    got = attn(*(_dev(t).expand(B, *t.shape[1:]) for t in (q, k, v)), causal, None if kl is None else _dev(kl[idx]))
    return A.check_elements(got, o[idx], w[idx], f"steps={steps} kv_len={kvs}")


def _attention(q, k, v, causal, kl):
    return ops.attention(q, k, v, causal=causal, kv_len=kl)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("case", A.LADDER_STREAM + A.LADDER_RESIDENT, ids=lambda c: "-".join(map(str, c[:6])))
def test_rescale_ladder(case, causal):
    res = case in A.LADDER_RESIDENT
    _note("resident" if res else "streaming", _run_ladder(case, causal, res, _attention))


# --------------------------------------------------------------------------- 4. peaked random, layouts, GQA
@pytest.mark.parametrize("want_resident", [False, True], ids=["streaming", "resident"])
@pytest.mark.parametrize("layout,ratio,scale", A.PEAKED_CONFIGS)
@pytest.mark.parametrize("Sq,Sk,D,causal", A.PEAKED_SHAPES)
def test_peaked_random_elements(Sq, Sk, D, causal, layout, ratio, scale, want_resident):
    B, H, Hkv = A.peaked_heads(ratio, want_resident)
    _expect_path(B, H, Sq, Sk, D, want_resident)
    bufs, views = A.peaked_layout(layout, B, Sq, Sk, H, Hkv, D)
    kl = A.random_kv_len(B, Sk, Sq)
    s = A.default_scale(D) if scale is None else scale
    o, w = A.ref64(*views(bufs), s, causal, kl)
    dbufs = _dev(bufs) if layout == "packed" else tuple(_dev(t) for t in bufs)
    q, k, v = views(dbufs)
    assert not q.is_contiguous()
    got = ops.attention(q, k, v, scale=scale, causal=causal, kv_len=_dev(kl))
    _note("resident" if want_resident else "streaming", A.check_elements(got, o, w))


# --------------------------------------------------------------------------- 5. out= views and sentinels
PATTERN = 0x5A5B                    # a finite bf16 (about 1.5e13) no attention output here can equal


@pytest.mark.parametrize("want_resident", [False, True], ids=["streaming", "resident"])
@pytest.mark.parametrize("pad", ["rows", "heads"])
@pytest.mark.parametrize("Sq", A.SENTINEL_SQ)
def test_out_view_and_sentinels(Sq, pad, want_resident):
    D, Sk = 64, Sq + 3
    B, H, Hkv = A.SENTINEL_HEADS[want_resident]
    _expect_path(B, H, Sq, Sk, D, want_resident)
    nb = 2                                                        # distinct batch entries, cycled over B
    q, k, v = A.peaked(nb, Sq, Sk, H, Hkv, D)
    o, w = A.ref64(q, k, v, A.default_scale(D), True, None)
    idx = torch.arange(B) % nb
    shape = (B, Sq + 2, H, D) if pad == "rows" else (B, Sq, H + 1, D)
    buf = torch.full(shape, PATTERN, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    view = buf[:, 1:Sq + 1] if pad == "rows" else buf[:, :, :H]
    inside = torch.zeros(shape, dtype=torch.bool, device=DEV)
    (inside[:, 1:Sq + 1] if pad == "rows" else inside[:, :, :H]).fill_(True)
    ret = ops.attention(_dev(q)[idx], _dev(k)[idx], _dev(v)[idx], causal=True, out=view)
    assert ret.data_ptr() == view.data_ptr()
    A.check_elements(view, o[idx], w[idx])
    outside = buf.view(torch.int16)[~inside]
    assert outside.numel() == buf.numel() - B * Sq * H * D
    assert bool((outside == PATTERN).all()), f"{int((outside != PATTERN).sum())} elements outside the out view changed"


# --------------------------------------------------------------------------- 6. attention_mx with a bf16 out
def _mx_call(q, k, v, causal, kl):
    B, Sq, H, D = q.shape
    o = torch.empty(B, Sq, H, D, device=DEV, dtype=torch.bfloat16)
    o8, os_ = ops.attention_mx(q, k, v, causal=causal, kv_len=kl, out=o)
    return o, o8, os_


@pytest.mark.parametrize("D", [64, 128])
def test_attention_mx_bf16_out_edges(D):
    Sq, Sk, causal = A.MX_PROBE[D]
    p = A.visibility_probe(Sq, Sk, 4, 2, D, A.kv_len_values(Sk))
    B = p["q"].shape[0]
    o, o8, os_ = _mx_call(_dev(p["q"]), _dev(p["k"]), _dev(p["v"]), causal, _dev(p["kv_len"]))
    A.check_visibility(o, p, causal, "attention_mx probe")
    dead = (A.visible(B, Sq, Sk, causal, p["kv_len"]).sum(-1) == 0).reshape(B * Sq)
    assert dead.any() and not dead.all()
    deq = ops.mx_dequant(o8.cpu(), os_.cpu())
    assert bool((deq[dead] == 0).all()), "o8 rows of fully masked queries must decode to zeros"
    of = o.float().cpu().reshape(B * Sq, -1)                      # e4m3: 3 mantissa bits below the block's amax
    assert bool(((deq - of).abs() <= 2.0 ** -3 * of.abs() + 1e-6).all())
    for causal in (False, True):
        _note("streaming", _run_ladder(A.MX_LADDER[D], causal, False, lambda *a: _mx_call(*a)[0]))
