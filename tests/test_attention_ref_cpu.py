"""tests/attention_ref.py (what tests/test_attention_edges_gpu.py compares the dense attention kernels
against) checked on the CPU: ref64 against the CPU path of ops.attention, the emulation of the kernels'
arithmetic against every check on every case table of the GPU file, and each planted bug (a mutant of the
emulation) against the check aimed at it -- so a GPU failure means the kernel, not the test.

The resident-kernel tables run here with fewer (batch, head) pairs of the same GQA ratio: every pair is
independent in the emulation, and the kv_len variants and probe passes that ride in the batch are kept.
"""
import pytest
import torch

import attention_ref as A
from lumen_amd import ops

VS_FP32_SHAPES = [(2, 257, 257, 16, 16, 64, False), (3, 77, 77, 8, 8, 64, True), (1, 197, 197, 12, 12, 64, False),
                  (2, 130, 130, 14, 2, 64, True), (1, 33, 300, 8, 2, 128, True), (2, 65, 65, 4, 4, 128, False),
                  (2, 20, 20, 4, 4, 32, False)]     # tests/test_kernels_gpu.py::test_attention_vs_fp32


def _vs_fp32_inputs(B, Sq, Sk, H, Hkv, D):
    g = torch.Generator().manual_seed(Sq * H + D)
    return (torch.randn(B, Sq, H, D, generator=g).bfloat16(), torch.randn(B, Sk, Hkv, D, generator=g).bfloat16(),
            torch.randn(B, Sk, Hkv, D, generator=g).bfloat16())


def _assert_one_ulp(o, w, got):
    """got (bf16, from the fp32 CPU path) is within one bf16 step of the fp64 result rounded to bf16.  The
    fp32 path's own error, a few 2^-24 of w = P @ |V|, can carry an element with cancellation (|o| << w)
    across more than one of its tiny steps: 2^-20 w is allowed on top."""
    ref = o.bfloat16().double()
    g = got.double()
    big = torch.maximum(ref.abs(), g.abs()).clamp_min(2.0 ** -126)
    ulp = torch.exp2(torch.floor(torch.log2(big)) - 7)
    assert ((g - ref).abs() <= ulp + 2.0 ** -20 * w).all()


# --------------------------------------------------------------------------- ref64 vs the op's CPU path
@pytest.mark.parametrize("B,Sq,Sk,H,Hkv,D,causal", VS_FP32_SHAPES)
def test_ref64_matches_cpu_op(B, Sq, Sk, H, Hkv, D, causal):
    q, k, v = _vs_fp32_inputs(B, Sq, Sk, H, Hkv, D)
    o, w = A.ref64(q, k, v, A.default_scale(D), causal, None)
    _assert_one_ulp(o, w, ops.attention(q, k, v, causal=causal))
    assert (w >= o.abs() - 1e-12).all()


def test_ref64_matches_cpu_op_kv_len():
    B, S, H, D = 3, 52, 12, 64
    qkv = torch.randn(B, S, 3, H, D, generator=torch.Generator().manual_seed(0)).bfloat16()
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    for kl in ([52, 10, 31], [0, 1, 60]):              # also: no key at all (zeros), kv_len past Sk (clamped)
        kl = torch.tensor(kl, dtype=torch.int32)
        o, w = A.ref64(q, k, v, A.default_scale(D), False, kl)
        _assert_one_ulp(o, w, ops.attention(q, k, v, kv_len=kl))
    # GQA, causal with Sq > Sk (rows without keys are zero) and a key-length mask together
    q, k, v = A.peaked(2, 9, 5, 6, 2, 32)
    kl = torch.tensor([5, 3], dtype=torch.int32)
    o, w = A.ref64(q, k, v, 0.1, True, kl)
    _assert_one_ulp(o, w, ops.attention(q, k, v, scale=0.1, causal=True, kv_len=kl))
    assert (o[:, :4] == 0).all() and (o[0, 4:] != 0).any()


# --------------------------------------------------------------------------- the GPU file's cases, shrunk
def _small_heads(H, Hkv):
    r = H // Hkv
    return (4, 4) if r == 1 else (2 * r, 2)


def vis_cases(stream_d=(32, 64, 128)):
    """(name, probe, causal) of both visibility tables and the attention_mx probes."""
    H, Hkv = A.VIS_STREAM_HEADS
    for D in stream_d:
        for causal in (False, True):
            for Sq, Sk in A.vis_stream_shapes():
                for kvs in (A.kv_len_values(Sk), None):
                    yield (f"stream D={D} causal={causal} Sq={Sq} Sk={Sk} kv={'set' if kvs else None}",
                           A.visibility_probe(Sq, Sk, H, Hkv, D, kvs), causal)
    for D, Sq, Sk, causal, _ in A.VIS_RESIDENT:
        for Hkv in (16, 4):
            assert A.resident(64, 16, Sq, Sk, D)
            h, hkv = _small_heads(16, Hkv)
            yield (f"resident D={D} causal={causal} Sq={Sq} Sk={Sk} Hkv={Hkv}",
                   A.visibility_probe(Sq, Sk, h, hkv, D, A.kv_len_values(Sk)), causal)
    for D, (Sq, Sk, causal) in A.MX_PROBE.items():
        yield f"mx D={D}", A.visibility_probe(Sq, Sk, 4, 2, D, A.kv_len_values(Sk)), causal


def ladder_cases():
    """(name, q, k, v, scale, causal, kv_len) of the ladder tables (one batch entry per distinct kv_len)."""
    for tab, res in ((A.LADDER_STREAM, False), (A.LADDER_RESIDENT, True), (list(A.MX_LADDER.values()), False)):
        for B, H, Hkv, Sq, Sk, D, steps, kvs in tab:
            assert A.resident(B, H, Sq, Sk, D) == res
            if res:
                H, Hkv = _small_heads(H, Hkv)
            nb = len(kvs) if kvs else 1
            scale = A.default_scale(D)
            q, k, v = A.ladder(1, Sq, Sk, H, Hkv, D, scale, steps)
            q, k, v = (t.expand(nb, *t.shape[1:]) for t in (q, k, v))
            for causal in (False, True):
                yield (f"ladder res={res} D={D} Sq={Sq} Sk={Sk} steps={steps} causal={causal} kv={kvs}",
                       q, k, v, scale, causal, None if kvs is None else torch.tensor(kvs, dtype=torch.int32))


def peaked_cases():
    for Sq, Sk, D, causal in A.PEAKED_SHAPES:
        for layout, ratio, scale in A.PEAKED_CONFIGS:
            B, H, Hkv = A.peaked_heads(ratio, False)
            bufs, views = A.peaked_layout(layout, B, Sq, Sk, H, Hkv, D)
            q, k, v = views(bufs)
            yield (f"peaked {layout} ratio={ratio} scale={scale} Sq={Sq} Sk={Sk} D={D}", q, k, v,
                   A.default_scale(D) if scale is None else scale, causal, A.random_kv_len(B, Sk, Sq))
    for Sq in A.SENTINEL_SQ:
        B, H, Hkv = A.SENTINEL_HEADS[False]
        q, k, v = A.peaked(B, Sq, Sq + 3, H, Hkv, 64)
        yield f"sentinel Sq={Sq}", q, k, v, A.default_scale(64), True, None


def _elem_fails(case, mutant):
    name, q, k, v, scale, causal, kl = case
    o, w = A.ref64(q, k, v, scale, causal, kl)
    try:
        A.check_elements(A.emulate(q, k, v, scale, causal, kl, mutant), o, w, name)
    except AssertionError:
        return True
    return False


def _vis_fails(case, mutant):
    name, p, causal = case
    try:
        A.check_visibility(A.emulate(p["q"], p["k"], p["v"], A.default_scale(p["D"]), causal, p["kv_len"], mutant),
                           p, causal, name)
    except AssertionError:
        return True
    return False


# --------------------------------------------------------------------------- the checks hold for the emulation
def test_emulation_passes_visibility():
    n = 0
    for name, p, causal in vis_cases():
        got = A.emulate(p["q"], p["k"], p["v"], A.default_scale(p["D"]), causal, p["kv_len"])
        A.check_visibility(got, p, causal, name)
        n += 1
    assert n > 500


def test_emulation_passes_elements():
    worst = 0.0
    for name, q, k, v, scale, causal, kl in list(ladder_cases()) + list(peaked_cases()):
        o, w = A.ref64(q, k, v, scale, causal, kl)
        worst = max(worst, A.check_elements(A.emulate(q, k, v, scale, causal, kl), o, w, name))
    print(f"worst ratio of the emulation to the check_elements bound: {worst:.3f}")
    assert 0.05 < worst <= 1.0


def test_probe_tables_cover_the_edges():
    """The kv_len set holds 0, 1, multiples of 64 and values leaving <= 16 live keys in the last chunk; the
    shapes hold Sq = 1, Sq > Sk under causal, and every probe pass is present."""
    kv = A.kv_len_values(257)
    assert kv[:2] == [0, 1] and {64, 128, 256, 257, 262} <= set(kv) and any(0 < x % 64 <= 16 for x in kv)
    shapes = A.vis_stream_shapes()
    assert (1, 1) in shapes and (1, 66) in shapes and (130, 60) in shapes and all(sk >= 1 for _, sk in shapes)
    p = A.visibility_probe(3, 70, 4, 2, 32, kv_lens=[70, 0])
    assert p["q"].shape[0] == 6 and p["t"].tolist() == [0, 1, 2, 0, 1, 2] and p["kv_len"].tolist() == [70] * 3 + [0] * 3
    assert p["v"].sum().item() == 2 * 70 * 2 and p["v"][1, 32 + 5, 1, 5] == 1 and (p["q"] == 0).all()


# --------------------------------------------------------------------------- each mutant fails its check
@pytest.mark.parametrize("mutant", ["no_o_rescale", "no_l_rescale"])
def test_rescale_mutants_fail_every_ladder_case(mutant):
    for case in ladder_cases():
        assert _elem_fails(case, mutant), case[0]


@pytest.mark.parametrize("mutant", ["causal_plus1", "kvlen_plus1", "kvlen_plus1_at_64", "dup_last_key"])
def test_mask_mutants_fail_visibility(mutant):
    for table in ("stream", "resident", "mx"):              # at least one case of each table catches it
        assert any(_vis_fails(c, mutant) for c in vis_cases(stream_d=(64,)) if c[0].startswith(table)), (mutant, table)


def test_gqa_mutant_fails_elements():
    hit = [c[0] for c in peaked_cases() if _elem_fails(c, "gqa_mod")]
    assert any("ratio=4" in n for n in hit) and any("ratio=7" in n for n in hit)
    for name, q, k, v, scale, causal, kl in peaked_cases():
        if "ratio=1" in name:
            assert torch.equal(A.emulate(q, k, v, scale, causal, kl, "gqa_mod"), A.emulate(q, k, v, scale, causal, kl))


# --------------------------------------------------------------------------- the gap this file records
@pytest.mark.parametrize("B,Sq,Sk,H,Hkv,D,causal", VS_FP32_SHAPES)
def test_randn_inputs_never_rescale(B, Sq, Sk, H, Hkv, D, causal):
    """On the randn inputs of test_attention_vs_fp32 no chunk after the first triggers the rescale: an
    emulation that never rescales o, or never rescales l, is bit-identical -- those tests cannot see it."""
    q, k, v = _vs_fp32_inputs(B, Sq, Sk, H, Hkv, D)
    base = A.emulate(q, k, v, A.default_scale(D), causal, None)
    for mutant in ("no_o_rescale", "no_l_rescale"):
        assert torch.equal(A.emulate(q, k, v, A.default_scale(D), causal, None, mutant), base)
    o, w = A.ref64(q, k, v, A.default_scale(D), causal, None)
    A.check_elements(base, o, w)
