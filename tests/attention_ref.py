"""References, input builders and per-element checks for the dense attention kernels
(csrc/attention.hip: the streaming attn_fwd_kernel and the K/V-resident attn_res_kernel).

Plain torch on the CPU; nothing here imports lumen_amd.  Tensors are laid out as the op takes them:
q ``[B, Sq, H, D]``, k / v ``[B, Sk, Hkv, D]``, out ``[B, Sq, H, D]``.

* :func:`ref64` -- float64 softmax attention on the bf16 inputs as given; also returns
  ``w = P @ |V|``, the weight the rounding-error bound of :func:`check_elements` scales with.
* :func:`visibility_probe` / :func:`check_visibility` -- an exact mask test: with q = 0 and a one-hot
  V every output element is ``1 / n_i`` or 0, so which keys a query saw can be read off its output row.
* :func:`ladder` -- inputs whose running row maximum moves by chosen amounts from one 64-key chunk to
  the next, so the lazy online-softmax rescale runs with factors below, at and above its threshold.
* :func:`emulate` -- the kernels' arithmetic (64-key chunks, fp32 scores, bf16 P, rescale only when
  some query of a 16-query wave grew by more than 8 log2 units) with optional deliberate bugs
  (:data:`MUTANTS`), which tests/test_attention_ref_cpu.py uses to show that the checks bite.
* the case tables of tests/test_attention_edges_gpu.py, shared with the CPU file so that every GPU
  case is known to pass on the emulation and to catch the mutants before it meets a kernel.
"""
from __future__ import annotations

import math

import torch

LOG2E = 1.4426950408889634
KC = 64                      # keys per chunk in both kernels
WAVE_Q = 16                  # queries per wave: the rescale decision is uniform over these

# check_elements: P is rounded to bf16 (2^-9 relative) in the numerator, the same rounded P forms the
# row sum, the output is rounded to bf16 (2^-9): 3 * 2^-9, doubled as the margin for accumulation
# order and the 1-ulp v_exp_f32 / v_rcp_f32.
ELEM_REL = 3 * 2.0 ** -8
ELEM_ABS = 1e-6

MUTANTS = ("no_o_rescale", "no_l_rescale", "causal_plus1", "kvlen_plus1", "kvlen_plus1_at_64", "gqa_mod",
           "dup_last_key")

# log2 units of running-max growth per unit step of k[..., 0], one per query of a 16-query wave: lanes
# below, at and above the threshold of 8, lanes whose alpha underflows to 0, lanes whose max falls
GAINS = (0., 1., 2., 4., 6., 7.5, 8., 8.5, 9., 12., 20., 40., 80., -8., -20., 3.)
STEPS_RISING = (0, 1, 2, 3, 4)
STEPS_NONMONO = (0, 2, 1, 3, 0)


# --------------------------------------------------------------------------- dispatch rule
def resident(B, H, Sq, Sk, D) -> bool:
    """attn_fwd takes the K/V-resident kernel (bf16 output only; attention_mx always streams)."""
    return B * H >= 1024 and -(-Sk // KC) * 2 * KC * D * 2 <= 80 * 1024 and Sq <= 1024


def resident_waves(Sq, D) -> int:
    return 8 if -(-Sq // 16) >= 10 and D >= 64 else 4


# --------------------------------------------------------------------------- masks
def _kv_tensor(kv_len, B, Sk):
    if kv_len is None:
        return torch.full((B,), Sk, dtype=torch.long)
    kl = torch.as_tensor(kv_len).long().reshape(B)
    return kl.clamp(max=Sk)


def visible(B, Sq, Sk, causal, kv_len) -> torch.Tensor:
    """bool [B, Sq, Sk]: key j is visible to query i.  kv_len is clamped to Sk; causal aligns the last
    query with the last key (j <= i + Sk - Sq)."""
    j = torch.arange(Sk)
    vis = (j.view(1, 1, Sk) < _kv_tensor(kv_len, B, Sk).view(B, 1, 1)).expand(B, Sq, Sk)
    if causal:
        vis = vis & (j.view(1, Sk) <= torch.arange(Sq).view(Sq, 1) + (Sk - Sq)).view(1, Sq, Sk)
    return vis


# --------------------------------------------------------------------------- float64 reference
def ref64(q, k, v, scale, causal, kv_len):
    """(o, w) float64 [B, Sq, H, D]: softmax attention of the inputs as given and w = P @ |V|.
    GQA by h // (H // Hkv); rows with no visible key are 0."""
    B, Sq, H, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    hk = torch.arange(H) // (H // Hkv)
    qd = q.detach().cpu().double().permute(0, 2, 1, 3)
    kd = k.detach().cpu().double().permute(0, 2, 1, 3)[:, hk]
    vd = v.detach().cpu().double().permute(0, 2, 1, 3)[:, hk]
    s = (qd @ kd.transpose(-1, -2)) * scale
    s = s.masked_fill(~visible(B, Sq, Sk, causal, kv_len).view(B, 1, Sq, Sk), float("-inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    p = p / p.sum(-1, keepdim=True).clamp_min(1e-300)
    return (p @ vd).permute(0, 2, 1, 3).contiguous(), (p @ vd.abs()).permute(0, 2, 1, 3).contiguous()


def check_elements(got, o, w, what="") -> float:
    """Assert |got - o| <= ELEM_REL * w + ELEM_ABS for every element; returns the worst ratio to the bound."""
    g = got.detach().cpu().double()
    assert g.shape == o.shape, (g.shape, o.shape)
    ratio = (g - o).abs() / (ELEM_REL * w + ELEM_ABS)
    ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, float("inf")))
    worst = ratio.max().item() if ratio.numel() else 0.0
    if not worst <= 1.0:
        b, i, h, d = (int(x) for x in torch.unravel_index(ratio.argmax(), ratio.shape))
        raise AssertionError(
            f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements over the bound; worst at "
            f"(b={b}, query={i}, head={h}, d={d}): got {g[b, i, h, d].item():.8g}, want {o[b, i, h, d].item():.8g}, "
            f"w {w[b, i, h, d].item():.4g}, {worst:.3g} x the bound")
    return worst


# --------------------------------------------------------------------------- visibility probe
def kv_len_values(Sk):
    """The key-length edges every mask table uses: 0, 1, around 16 (the short-tail path), around the
    64-key chunk boundaries, Sk - 1, Sk and a value past Sk (clamped)."""
    vals = [0, 1, 15, 16, 17, 63, 64, 65, 80, 81, 128, Sk - 1, Sk]
    out = []
    for x in vals:
        if 0 <= x <= Sk and x not in out:
            out.append(x)
    return out + [Sk + 5]


def visibility_probe(Sq, Sk, H, Hkv, D, kv_lens=None, B=None, start=0, seed=0):
    """Inputs of the exact mask test.  q = 0; k random (it must not matter: one [1, Sk, Hkv, D] block
    broadcast over the batch); v a one-hot code: batch entry b carries pass t_b, with v[b, j, :, d] = 1
    iff j == t_b * D + d.  Every visible score is 0 and every p exactly 1, so out[b, i, h, d] is 1 / n_i
    if key t_b * D + d is visible to query i and 0 otherwise.

    The ceil(Sk / D) passes and the ``kv_lens`` variants ride in the batch: entry b is pair
    ``(start + b) % (passes * variants)`` of the (variant-major) pair list; B defaults to all pairs.
    Returns dict(q, k, v, kv_len (int32 [B] or None), t (long [B]), Sq, Sk, D)."""
    T = -(-Sk // D)
    nv = 1 if kv_lens is None else len(kv_lens)
    B = T * nv if B is None else B
    pair = (start + torch.arange(B)) % (T * nv)
    t = pair % T
    g = torch.Generator().manual_seed(seed * 7919 + Sq * 131 + Sk)
    k = (4.0 * torch.randn(1, Sk, Hkv, D, generator=g)).bfloat16().expand(B, Sk, Hkv, D)
    dj = torch.arange(Sk).view(1, Sk) - (t * D).view(B, 1)                      # the d that key j codes
    v = (dj.view(B, Sk, 1, 1) == torch.arange(D).view(1, 1, 1, D)).expand(B, Sk, Hkv, D).to(torch.bfloat16)
    kl = None if kv_lens is None else torch.tensor(kv_lens, dtype=torch.int32)[pair // T]
    return dict(q=torch.zeros(B, Sq, H, D, dtype=torch.bfloat16), k=k, v=v.contiguous(), kv_len=kl, t=t,
                Sq=Sq, Sk=Sk, D=D)


def check_visibility(got, probe, causal, what=""):
    """Elements of invisible keys are bit-exact zero (so rows with no visible key are all zero, without a
    NaN); the others are within 2^-8 / n_i of 1 / n_i (one bf16 rounding of the output and the 1-ulp
    reciprocal).  A key counted twice puts 2 / (n_i + 1) where its own 1 / n_i belongs."""
    g = got.detach().cpu()
    B, Sq, H, D = g.shape
    Sk = probe["Sk"]
    vis = visible(B, Sq, Sk, causal, probe["kv_len"])
    n = vis.sum(-1)                                                              # [B, Sq]
    key = probe["t"].view(B, 1) * D + torch.arange(D).view(1, D)                 # [B, D]
    seen = torch.gather(vis, 2, key.clamp(max=Sk - 1).view(B, 1, D).expand(B, Sq, D)) & (key < Sk).view(B, 1, D)
    seen = seen.view(B, Sq, 1, D).expand(B, Sq, H, D)
    bits = g.contiguous().view(torch.int16)
    bad0 = (bits != 0) & ~seen
    if bad0.any():
        b, i, h, d = (int(x) for x in bad0.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad0.sum())} elements of invisible keys are not +0; first at (b={b}, "
                             f"query={i}, head={h}, d={d}) = key {int(key[b, d])}: got {g[b, i, h, d].item()!r} "
                             f"(kv_len {None if probe['kv_len'] is None else int(probe['kv_len'][b])}, n_i {int(n[b, i])})")
    assert not torch.isnan(g.float()).any(), f"{what}: NaN in the output"
    want = (1.0 / n.double().clamp_min(1)).view(B, Sq, 1, 1).expand(B, Sq, H, D)
    bad1 = ((g.double() - want).abs() > 2.0 ** -8 * want) & seen
    if bad1.any():
        b, i, h, d = (int(x) for x in bad1.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad1.sum())} elements of visible keys are off 1 / n_i; first at (b={b}, "
                             f"query={i}, head={h}, d={d}) = key {int(key[b, d])}: got {g[b, i, h, d].item()!r}, "
                             f"n_i {int(n[b, i])}, want {want[b, i, h, d].item():.8g}")


# --------------------------------------------------------------------------- inputs that drive the rescale
def ladder(B, Sq, Sk, H, Hkv, D, scale, steps, seed=0):
    """k[..., 0] = steps[chunk % len(steps)] (a step function of the 64-key chunk index), q[i, :, 0] =
    GAINS[i % 16] / (scale * log2 e): the running max of row i, in the kernel's log2 units, moves by
    GAINS[i % 16] per unit step.  The other dimensions are 0.5 * randn; v is randn."""
    g = torch.Generator().manual_seed(seed * 7919 + Sq * 131 + Sk + D)
    q = 0.5 * torch.randn(B, Sq, H, D, generator=g)
    k = 0.5 * torch.randn(B, Sk, Hkv, D, generator=g)
    v = torch.randn(B, Sk, Hkv, D, generator=g)
    st = torch.tensor(steps, dtype=torch.float32)
    k[..., 0] = st[(torch.arange(Sk) // KC) % len(steps)].view(1, Sk, 1)
    q[..., 0] = (torch.tensor(GAINS)[torch.arange(Sq) % WAVE_Q] / (scale * LOG2E)).view(1, Sq, 1)
    return q.bfloat16(), k.bfloat16(), v.bfloat16()


def peaked(B, Sq, Sk, H, Hkv, D, seed=0):
    """q, k = 2 * randn (a peaked softmax: a mis-addressed key or value row moves single elements), v = randn."""
    g = torch.Generator().manual_seed(seed * 7919 + Sq * 131 + Sk + H)
    return ((2 * torch.randn(B, Sq, H, D, generator=g)).bfloat16(),
            (2 * torch.randn(B, Sk, Hkv, D, generator=g)).bfloat16(),
            torch.randn(B, Sk, Hkv, D, generator=g).bfloat16())


# --------------------------------------------------------------------------- emulation of the kernels
def emulate(q, k, v, scale, causal, kv_len, mutant=None):
    """The kernels' arithmetic on the CPU, bf16 [B, Sq, H, D]: 64-key chunks over K/V padded with copies of
    row Sk - 1 (as staged), fp32 scores, running max in log2 units, P = exp2(s * scale_log2 - m) rounded to
    bf16 for both the PV product and the row sum, fp32 accumulators, and o / l rescaled only in chunks where
    some query of the 16-query wave (the ragged block's clamped rows included) has a max that grew by more
    than 8.  Skipped chunks and the resident kernel's 16-key tail step equal fully masked chunks here.
    ``mutant`` plants one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS, mutant
    B, Sq, H, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    hk = torch.arange(H) % Hkv if mutant == "gqa_mod" else torch.arange(H) // (H // Hkv)
    nblk = -(-Sq // WAVE_Q)
    Sqp = nblk * WAVE_Q
    Skp = (Sk // KC + 1) * KC                                     # at least one staged row past Sk
    qrow = torch.arange(Sqp).clamp(max=Sq - 1)
    krow = torch.arange(Skp).clamp(max=Sk - 1)
    qf = q.detach().cpu().float().permute(0, 2, 1, 3)[:, :, qrow]             # [B, H, Sqp, D]
    kf = k.detach().cpu().float().permute(0, 2, 1, 3)[:, hk][:, :, krow]      # [B, H, Skp, D]
    vf = v.detach().cpu().float().permute(0, 2, 1, 3)[:, hk][:, :, krow]
    kl = _kv_tensor(kv_len, B, Sk)
    if mutant == "kvlen_plus1":
        kl = kl + 1
    elif mutant == "kvlen_plus1_at_64":
        kl = kl + (kl % KC == 0).long()
    j = torch.arange(Skp)
    vis = (j.view(1, 1, Skp) < kl.view(B, 1, 1)).expand(B, Sqp, Skp)
    if causal:
        off = Sk - Sq + (1 if mutant == "causal_plus1" else 0)
        vis = vis & (j.view(1, Skp) <= torch.arange(Sqp).view(Sqp, 1) + off).view(1, Sqp, Skp)
    if mutant == "dup_last_key" and Sk % KC:
        vis = vis.clone()
        vis[:, :, Sk] = vis[:, :, Sk - 1]                        # the clamped copy right after the last key
    vis = vis.view(B, 1, Sqp, Skp)
    sl2 = torch.tensor(scale * LOG2E, dtype=torch.float32)
    ninf = float("-inf")
    o = torch.zeros(B, H, Sqp, D)
    l = torch.zeros(B, H, Sqp, 1)
    m = torch.full((B, H, Sqp, 1), ninf)
    for c in range(Skp // KC):
        ks = slice(c * KC, (c + 1) * KC)
        s = (qf @ kf[:, :, ks].transpose(-1, -2)).masked_fill(~vis[..., ks], ninf)
        mcand = torch.maximum(m, s.amax(-1, keepdim=True) * sl2)
        trig = (mcand > m + 8.0).view(B, H, nblk, WAVE_Q).any(-1, keepdim=True).expand(B, H, nblk, WAVE_Q)
        trig = trig.reshape(B, H, Sqp, 1)
        alpha = torch.exp2(m - torch.where(mcand == ninf, torch.zeros_like(mcand), mcand))
        alpha = torch.where(trig, alpha, torch.ones_like(alpha))
        if mutant != "no_o_rescale":
            o = o * alpha
        if mutant != "no_l_rescale":
            l = l * alpha
        m = torch.where(trig, mcand, m)
        p = torch.exp2(s * sl2 - torch.where(m == ninf, torch.zeros_like(m), m)).bfloat16().float()
        o = o + p @ vf[:, :, ks]
        l = l + p.sum(-1, keepdim=True)
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    return (o * inv)[:, :, :Sq].permute(0, 2, 1, 3).bfloat16().contiguous()


# --------------------------------------------------------------------------- case tables (GPU file + CPU file)
VIS_STREAM_SQ = (1, 16, 17, 64, 65, 130)
VIS_STREAM_DELTA = (-70, -17, -1, 0, 1, 63, 64, 65)                # Sk - Sq, where Sk >= 1
VIS_STREAM_HEADS = (4, 2)


def vis_stream_shapes():
    return [(Sq, Sq + d) for Sq in VIS_STREAM_SQ for d in VIS_STREAM_DELTA if Sq + d >= 1]


# (D, Sq, Sk, causal, clean_chunks): B = 64, H = 16, each with Hkv 16 and 4.  clean_chunks is the
# TUNE_ATTN_CLEAN_CHUNKS arm (1 = the default mask-free clean chunks, 0 = every chunk masked).
VIS_RESIDENT = [(D, Sq, Sk, causal, 1)
                for D, shapes in ((64, ((48, 77), (150, 257), (1, 197), (150, 320))),
                                  (128, ((48, 128), (150, 81))),
                                  (32, ((48, 640), (17, 65))))
                for Sq, Sk in shapes for causal in (False, True)]
VIS_RESIDENT += [(64, 33, 100, True, 1), (64, 100, 33, True, 1)]
VIS_RESIDENT += [(64, Sq, Sk, causal, 0) for Sq, Sk in ((150, 257), (48, 77)) for causal in (False, True)]

# (B, H, Hkv, Sq, Sk, D, steps, kv_lens): kv_lens None = no key-length mask, else one value per batch entry
# (cycled); the batch entries share q, k, v.  Each step table's largest value sits in a chunk that one
# kv_len ends inside.
LADDER_STREAM = [
    (1, 2, 1, 48, 320, 64, STEPS_RISING, None),
    (1, 2, 1, 48, 320, 64, STEPS_NONMONO, None),
    (2, 2, 1, 48, 320, 64, STEPS_RISING, (300, 320)),             # 300: inside chunk 4, the largest step
    (1, 2, 1, 48, 256, 128, STEPS_RISING, None),
    (1, 2, 1, 48, 256, 128, STEPS_NONMONO, None),
    (1, 2, 1, 80, 336, 32, STEPS_RISING, None),
    (1, 2, 1, 80, 336, 32, STEPS_NONMONO, None),
]
LADDER_RESIDENT = [
    (64, 16, 16, 48, 320, 64, STEPS_RISING, (320, 300, 257, 192)),
    (64, 16, 4, 150, 320, 64, STEPS_NONMONO, (320, 200, 129, 64)),  # 200: inside chunk 3, the largest step
    (64, 16, 16, 150, 320, 64, STEPS_RISING, None),
    (64, 16, 4, 48, 128, 128, (0, 1), (128, 100, 65, 80)),
    (64, 16, 16, 48, 128, 128, (1, 0), None),
    (64, 16, 16, 48, 640, 32, STEPS_RISING, (640, 630, 577, 320)),
    (64, 16, 4, 48, 640, 32, STEPS_NONMONO, None),
]

# (Sq, Sk, D, causal) of the peaked-random and layout test, each run on both kernels
PEAKED_SHAPES = [(70, 150, 64, True), (33, 81, 128, False), (50, 50, 32, True), (1, 197, 64, False)]
# (layout, H // Hkv, scale): "packed" = views of one [B, S, 3, H, D] projection (H = Hkv), "llm" =
# q5[:, :, :H] of a [B, T, H + 2 Hkv, D] projection with separately allocated k and v
PEAKED_CONFIGS = [("packed", 1, None), ("llm", 4, 0.5), ("llm", 7, 0.03), ("llm", 1, None)]


def peaked_heads(ratio, want_resident):
    """(B, H, Hkv) of a peaked case: B * H >= 1024 for the resident kernel, a handful otherwise."""
    if not want_resident:
        return 2, 2 * ratio, 2
    return (40, 28, 4) if ratio == 7 else (64, 16, 16 // ratio)


def peaked_layout(layout, B, Sq, Sk, H, Hkv, D, seed=0):
    """q, k, v of :func:`peaked` placed as strided views of their projections' buffers."""
    q, k, v = peaked(B, Sq, Sk, H, Hkv, D, seed)
    if layout == "packed":
        assert H == Hkv
        buf = torch.zeros(B, max(Sq, Sk), 3, H, D, dtype=torch.bfloat16)
        buf[:, :Sq, 0], buf[:, :Sk, 1], buf[:, :Sk, 2] = q, k, v
        return buf, (lambda t: (t[:, :Sq, 0], t[:, :Sk, 1], t[:, :Sk, 2]))
    buf = torch.zeros(B, Sq, H + 2 * Hkv, D, dtype=torch.bfloat16)
    buf[:, :, :H] = q
    return (buf, k, v), (lambda t: (t[0][:, :, :H], t[1], t[2]))


# out= views with sentinels: Sq (a ragged last 16-query block each), Sk = Sq + 3, D = 64, causal
SENTINEL_SQ = (1, 17, 65, 257)
SENTINEL_HEADS = {False: (2, 4, 2), True: (64, 16, 4)}              # want_resident -> (B, H, Hkv)

# attention_mx with a bf16 out (always the streaming kernel): per D one probe (Sq, Sk, causal; H = 4,
# Hkv = 2) whose kv_len set leaves some queries without keys, and one ladder case
MX_PROBE = {64: (65, 130, True), 128: (17, 81, True)}
MX_LADDER = {64: (2, 4, 2, 48, 320, 64, STEPS_RISING, (300, 320)),
             128: (1, 2, 1, 48, 256, 128, STEPS_NONMONO, None)}


def random_kv_len(B, Sk, seed):
    g = torch.Generator().manual_seed(seed * 31 + Sk)
    return torch.randint(0, Sk + 1, (B,), generator=g, dtype=torch.int32)


def default_scale(D):
    return 1.0 / math.sqrt(D)
