"""The device sampler op (csrc/sampler.hip) against its CPU reference (ops.llm.sample_rows):
candidates, token and bitmap exactly, and row_topk's results bit for bit on a plain greedy batch."""
import functools

import numpy as np
import pytest
import torch

from lumen_amd import ops
from lumen_amd.ops import llm as lops

pytestmark = pytest.mark.gpu
DEV = "cuda"
K = 64
# 1,000: one launch.  20,481: five 4096-column chunks + a one-column chunk, and V % 32 = 1, so the
# last bitmap word is partial.  151,936: the Qwen2 vocabulary.
SIZES = [1000, 20481, 151936]
U_LAST = 1.0 - 2.0 ** -53


def _logits(V, B, seed):
    """distinct by construction: per row a seeded permutation of an arithmetic sequence over [-12, 12]"""
    base = torch.linspace(-12, 12, V, dtype=torch.float64).float()
    g = torch.Generator().manual_seed(seed)
    return torch.stack([base[torch.randperm(V, generator=g)] for _ in range(B)])


def _bitmap_rows(S, V, sets, junk_rows=()):
    seen = np.zeros((S, lops.seen_words(V)), np.uint32)
    for slot, toks in sets.items():
        for t in toks:
            seen[slot, t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    g = np.random.default_rng(V)
    for r in junk_rows:     # a slot no row of the launch uses: must come back untouched
        seen[r] = g.integers(0, 2 ** 32, seen.shape[1], dtype=np.uint32)
        if V % 32:
            seen[r, -1] &= np.uint32((1 << (V % 32)) - 1)
    return torch.from_numpy(seen.view(np.int32).copy())


def _transformed(logits, rows, seen_sets):
    """the host composition (rep_penalty_ + multiply) of every row, for the distinctness check"""
    x = logits.clone()
    ids = [sorted(seen_sets.get(r["slot"], set()) | {r["in_id"]}) if r["slot"] >= 0 else [] for r in rows]
    lops.rep_penalty_(x, ids, [r["pen"] for r in rows])
    x.mul_(torch.tensor([r["inv_t"] for r in rows], dtype=torch.float32)[:, None])
    return x


def _masses(v, lse, top_p=None):
    """fp64 candidate masses of one reference row: (c, what top_p is compared with)"""
    c = np.cumsum(np.exp(v.numpy().astype(np.float64) - np.float64(lse)))
    return c, (c / c[-1] if top_p is None or c[-1] < top_p else c)


def _ref(logits, rows, seen, u=None):
    B = len(rows)
    return lops.sample_rows(logits, [r["inv_t"] for r in rows], [r["top_p"] for r in rows],
                            [r["pen"] for r in rows], u if u is not None else [0.0] * B,
                            [r["greedy"] for r in rows], [r["slot"] for r in rows], seen.clone(),
                            [r["in_id"] for r in rows])


def _mid_u(v, lse, top_p, m=None):
    """(u, candidate) with u the midpoint of candidate m's cdf interval (>= 1e-6 wide) of a reference row"""
    c, _ = _masses(v, lse)
    n = int(np.searchsorted(c, top_p * c[-1] if c[-1] < top_p else top_p) + 1)
    n = max(1, min(n, K))
    cdf = c[:n] / c[n - 1]
    m = n // 2 if m is None else min(m, n - 1)
    lo = cdf[m - 1] if m > 0 else 0.0
    assert cdf[m] - lo >= 1e-6
    return 0.5 * (lo + cdf[m]), m


def _mid_top_p(v, lse, m, normalised):
    """top_p halfway between two consecutive cumulative masses >= 1e-3 apart (those top_p is compared with:
    c_j, or c_j / c_63 when the 64 candidates hold less than top_p), so that the nucleus is m + 2 long"""
    c, _ = _masses(v, lse)
    q = c / c[-1] if normalised else c
    assert q[m + 1] - q[m] >= 1e-3
    tp = 0.5 * (q[m] + q[m + 1])
    assert (c[-1] < tp) == normalised
    return float(tp)


@functools.lru_cache(maxsize=None)
def _case(V):
    """inputs and the CPU reference of one vocabulary size, computed once: the five rows of the main
    launch and four more (u = 0, u = 1 - 2^-53, top_p at two midpoints)"""
    logits = _logits(V, 9, seed=V)
    order = logits.argsort(dim=1, descending=True)
    top = lambda b, j: int(order[b, j])  # noqa: E731
    neg = lambda b: int(order[b, V - 7])  # noqa: E731  (a negative logit)
    rows = [
        dict(greedy=1, inv_t=1.0, top_p=1.0, pen=1.0, slot=2, in_id=top(0, 3)),                  # greedy
        dict(greedy=1, inv_t=1.0, top_p=1.0, pen=1.3, slot=0, in_id=top(1, 1)),                  # greedy, penalty
        dict(greedy=0, inv_t=1 / 0.9, top_p=0.95, pen=1.0, slot=4, in_id=top(2, 2)),             # sampled
        dict(greedy=0, inv_t=1 / 0.8, top_p=0.9, pen=1.2, slot=1, in_id=top(3, 1)),              # sampled, penalty
        dict(greedy=0, inv_t=1 / 0.7, top_p=1.0, pen=1.3, slot=-1, in_id=top(4, 0)),             # no slot
        dict(greedy=0, inv_t=1.0, top_p=0.9, pen=1.1, slot=6, in_id=top(5, 5)),                  # u = 0
        dict(greedy=0, inv_t=1.0, top_p=0.85, pen=1.0, slot=-1, in_id=top(6, 0)),                # u = 1 - 2^-53
        dict(greedy=0, inv_t=1 / 0.6, top_p=None, pen=1.2, slot=7, in_id=top(7, 2)),             # top_p midpoints
        dict(greedy=0, inv_t=1 / 1.3, top_p=None, pen=1.0, slot=-1, in_id=top(8, 4)),
    ]
    # seen sets: the largest logit, a negative one, id 0, id V - 1; in_ids[b] is NOT in the bitmap
    sets = {r["slot"]: {top(b, 0), top(b, 6), neg(b), 0, V - 1} - {r["in_id"]} for b, r in enumerate(rows) if r["slot"] >= 0}
    seen = _bitmap_rows(8, V, sets, junk_rows=(3, 5))
    x = _transformed(logits, rows, sets)
    t65 = torch.topk(x, K + 1, dim=1).values
    assert bool((t65[:, :-1] > t65[:, 1:]).all()), "transformed top-65 values must be distinct: change the seed"
    # pass 1: candidates and lse (they do not depend on u / top_p); then place top_p and u
    for r in rows[7:]:
        r["top_p"] = 1.0
    v, i, lse, _, _ = _ref(logits, rows, seen)
    rows[7]["top_p"] = _mid_top_p(v[7], lse[7], 20, normalised=False) if V == 1000 else \
        _mid_top_p(v[7], lse[7], 20, normalised=True)
    rows[8]["top_p"] = _mid_top_p(v[8], lse[8], 40, normalised=True)
    for b, r in enumerate(rows):      # the literal top_p of the other rows must not sit on a mass either
        if not r["greedy"] and r["top_p"] < 1.0:
            _, q = _masses(v[b], lse[b], r["top_p"])
            assert np.abs(q - r["top_p"]).min() >= 5e-4, (b, "top_p too close to a cumulative mass: change it")
    u, want = [0.0] * 9, [0] * 9
    for b, r in enumerate(rows):
        if r["greedy"]:
            continue
        if b == 5:
            u[b], want[b] = 0.0, 0
        elif b == 6:
            c, _ = _masses(v[b], lse[b])
            tp = r["top_p"]
            n = max(1, min(int(np.searchsorted(c, tp * c[-1] if c[-1] < tp else tp) + 1), K))
            u[b], want[b] = U_LAST, n - 1
        else:
            u[b], want[b] = _mid_u(v[b], lse[b], r["top_p"], m=None if b != 4 else 37)
    ref = _ref(logits, rows, seen, u=u)
    assert [int(t) for t in ref[3]] == [int(i[b, want[b]]) for b in range(9)]
    assert want[7] <= 21 and rows[8]["top_p"] < 1.0
    return logits, rows, seen, u, ref


@pytest.mark.parametrize("V", SIZES)
@pytest.mark.parametrize("sel", [(0, 1, 2, 3, 4), (5, 6, 7, 8)], ids=["main5", "edges4"])
def test_op_matches_reference(V, sel):
    logits, rows, seen, u, ref = _case(V)
    sel = list(sel)
    d_logits = logits[sel].to(DEV)
    keep = d_logits.clone()
    sub = [rows[b] for b in sel]
    d_seen = seen.to(DEV)
    out_ids = torch.full((len(sel),), -7, dtype=torch.long, device=DEV)
    v, i, lse, tok, seen2 = lops.sample_rows(d_logits, [r["inv_t"] for r in sub], [r["top_p"] for r in sub],
                                             [r["pen"] for r in sub], [u[b] for b in sel],
                                             [r["greedy"] for r in sub], [r["slot"] for r in sub], d_seen,
                                             [r["in_id"] for r in sub], out_ids=out_ids)
    torch.cuda.synchronize()
    rv, ri, rlse, rtok, _ = ref
    # the reference bitmap of this selection: only the selected rows mark their input token
    rseen = lops.sample_rows(logits[sel], [r["inv_t"] for r in sub], [r["top_p"] for r in sub],
                             [r["pen"] for r in sub], [u[b] for b in sel], [r["greedy"] for r in sub],
                             [r["slot"] for r in sub], seen.clone(), [r["in_id"] for r in sub])[4]
    assert torch.equal(d_logits, keep), "the logits are read only"
    assert torch.equal(v.cpu(), rv[sel])
    assert torch.equal(i.cpu(), ri[sel])
    # rtol 1e-5 is the relative bound test_kernels_gpu.py puts on row_topk's lse
    assert torch.allclose(lse.cpu(), rlse[sel], rtol=1e-5, atol=0)
    assert torch.equal(tok.cpu(), rtok[sel])
    assert torch.equal(out_ids.cpu(), rtok[sel].long())
    assert torch.equal(seen2.cpu(), rseen)
    assert not torch.equal(rseen, seen), "the inputs were to be marked"


@pytest.mark.parametrize("V", SIZES)
def test_tokens_without_the_candidate_outputs(V):
    """the decode graph's call: no candidate outputs, so greedy rows run a single merge round"""
    logits, rows, seen, u, ref = _case(V)
    B = len(rows)
    out_ids = torch.full((B,), -7, dtype=torch.long, device=DEV)
    v, i, lse, tok, seen2 = lops.sample_rows(logits.to(DEV), [r["inv_t"] for r in rows], [r["top_p"] for r in rows],
                                             [r["pen"] for r in rows], u, [r["greedy"] for r in rows],
                                             [r["slot"] for r in rows], seen.to(DEV), [r["in_id"] for r in rows],
                                             out_ids=out_ids, candidates=False)
    torch.cuda.synchronize()
    assert v is None and i is None and lse is None
    assert torch.equal(tok.cpu(), ref[3])
    assert torch.equal(out_ids.cpu(), ref[3].long())
    assert torch.equal(seen2.cpu(), ref[4])


@pytest.mark.parametrize("V", SIZES)
def test_plain_greedy_batch_is_row_topk_bit_for_bit(V):
    logits = torch.cat([_case(V)[0][:3], torch.randn(2, V, generator=torch.Generator().manual_seed(V)) * 4]).to(DEV)
    B = logits.shape[0]
    seen = torch.zeros((1, lops.seen_words(V)), dtype=torch.int32, device=DEV)
    v, i, lse, tok, seen = lops.sample_rows(logits, [1.0] * B, [1.0] * B, [1.0] * B, [0.5] * B, [1] * B, [-1] * B,
                                            seen, [1] * B)
    tv, ti, tlse = ops.row_topk(logits, K, with_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(v.view(torch.int32), tv.view(torch.int32))
    assert torch.equal(i, ti)
    assert torch.equal(lse.view(torch.int32), tlse.view(torch.int32))
    assert torch.equal(tok, ti[:, 0])
    assert not seen.any()
