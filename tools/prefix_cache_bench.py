"""Prefix KV cache benchmark: what a second turn about the same image costs with and without it.

Mirrors tools/vlm_bench.py (random-weight LLaVA-Llama-3-8B preset, fp8 weights, one synthetic
1024x768 JPEG per conversation) and measures

 (a) time to first token of turn 1 (cold: a new image) and turn 2 (same image, one more user
     turn) with the prefix cache on and off.  The request path is the VLM service's
     (services/vlm/backend.py:_submit): hash + match before the JPEG decode; a hit that covers the
     image rows skips decode, encode-ahead and the vision tower;
 (b) the host time of hashing the JPEG and building the block keys (paid by every request when
     the cache is on);
 (c) the paged-prefill kernel against the gather path (LUMEN_PAGED_PREFILL=0: index_select of
     the prefix, transposing copy, widening copy, flash kernel) for one 8B layer shape
     (H=32, Hkv=8, D=128), bf16 and fp8 caches, cache-cold (every call reads a block set the
     previous calls did not touch; the pools are larger than the Infinity Cache).

usage: python tools/prefix_cache_bench.py [--n 10] [--iters 40] [--skip-ttft] [--skip-kernel] [--rows-sweep]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lumen_amd import ops  # noqa: E402
from lumen_amd._native import load_hip  # noqa: E402
from lumen_amd.models.vlm import ENCODE_AHEAD, VLM, VLM_PRESETS, PreparedPrefill  # noqa: E402
from lumen_amd.ops import llm as lops  # noqa: E402
from lumen_amd.runtime.engine import LLMEngine, SamplingParams  # noqa: E402
from lumen_amd.runtime.kv_cache import PagedKVCache  # noqa: E402
from lumen_amd.services.vlm.backend import CachedImagePrefill, prefix_cache_keys  # noqa: E402
from lumen_amd.utils.h2d import h2d_ahead  # noqa: E402
from lumen_amd.utils.image import encode_jpeg  # noqa: E402
from lumen_amd.utils.jpeg import decode_image  # noqa: E402
from tools.face_ocr_bench import synth_image  # noqa: E402

SHAPES = ((576, 48), (640, 128), (2048, 2048), (6144, 2048))      # (start_pos, T)


# ----------------------------------------------------------------------------- (c) kernel vs gather
def gather_attention(qkv, kc, vc, blocks, start_pos, H, Hkv, D):
    """the start_pos > 0 gather branch of LLM.prefill (models/llm.py), step for step"""
    T = qkv.shape[0]
    S = start_pos + T
    q5 = qkv.view(1, T, H + 2 * Hkv, D)
    k_all, v_all = lops.gather_kv(kc, vc, blocks, S)
    k_all = k_all.to(qkv.dtype).unsqueeze(0)
    v_all = v_all.to(qkv.dtype).unsqueeze(0).contiguous()
    return ops.attention(q5[:, :, :H], k_all, v_all, causal=True).view(T, H * D)


def kernel_bench(iters: int, shapes=SHAPES) -> list[dict]:
    dev = torch.device("cuda")
    H, Hkv, D = 32, 8, 128
    max_nb = max(128, max(-(-(s + t) // 64) for s, t in shapes))
    NB = 16 * max_nb                         # 2048 blocks: the two pools hold 536 MB (bf16) / 268 MB (fp8) > 256 MiB
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for dtype in (torch.bfloat16, torch.float8_e4m3fn):
        kc = (torch.randn(NB, Hkv, 64, D, generator=g, device=dev, dtype=torch.bfloat16) * 0.5).to(dtype)
        vc = (torch.randn(NB, Hkv, D, 64, generator=g, device=dev, dtype=torch.bfloat16) * 0.5).to(dtype)
        perm = torch.randperm(NB, generator=g, device=dev)
        for start, T in shapes:
            nb = -(-(start + T) // 64)
            # disjoint block lists over the whole pool, used in turn: a list comes back only after
            # every other block of both pools has been read
            lists = [perm[i * nb:(i + 1) * nb].long() for i in range(NB // nb)]
            sets = len(lists)
            qkv = torch.randn(T, (H + 2 * Hkv) * D, generator=g, device=dev, dtype=torch.bfloat16)
            out = torch.empty(T, H * D, device=dev, dtype=torch.bfloat16)
            fns = {"kernel": lambda b: lops.paged_prefill(qkv, kc, vc, b, start, H, Hkv, out=out),
                   "gather": lambda b: gather_attention(qkv, kc, vc, b, start, H, Hkv, D)}
            a, b = fns["kernel"](lists[0]), fns["gather"](lists[0])
            torch.cuda.synchronize()
            rel = ((a.float() - b.float()).norm() / b.float().norm()).item()
            ms = {"kernel": [], "gather": []}
            for rnd in range(4):             # alternate the two paths; each call on the next block set
                name = ("kernel", "gather")[rnd % 2]
                for i in range(iters // 2 + 2):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fns[name](lists[(rnd * (iters // 2 + 2) + i) % sets])
                    e1.record()
                    e1.synchronize()
                    if i >= 2:               # the first two calls of a round warm the path up
                        ms[name].append(e0.elapsed_time(e1))
            row = {"what": "paged_prefill kernel vs gather path", "H": H, "Hkv": Hkv, "D": D,
                   "kv": "fp8" if dtype == torch.float8_e4m3fn else "bf16", "start_pos": start, "T": T,
                   "kernel_ms": float(np.median(ms["kernel"])), "gather_ms": float(np.median(ms["gather"])),
                   "kernel_p90_ms": float(np.percentile(ms["kernel"], 90)),
                   "gather_p90_ms": float(np.percentile(ms["gather"], 90)),
                   "calls_each": len(ms["kernel"]), "rel_diff": rel}
            row["kernel_over_gather"] = row["kernel_ms"] / row["gather_ms"]
            print(json.dumps(row), flush=True)
            rows.append(row)
        del kc, vc
    return rows


# ----------------------------------------------------------------------------- (a) + (b) TTFT
def ttft_bench(args) -> dict:
    dev = torch.device("cuda")
    cfg = VLM_PRESETS[args.preset]
    m = VLM(cfg, device=dev)
    m.random_init(0)
    if not args.bf16:
        m.quantize_fp8()
    torch.cuda.synchronize()
    N = cfg.num_image_tokens
    V = cfg.llm.vocab_size
    rng = np.random.default_rng(0)
    jpegs = [encode_jpeg(synth_image(rng, 768, 1024, "photo")) for _ in range(args.n + args.warmup)]
    text = [int(t) for t in rng.integers(1000, min(V, 30000), 48 + 16 + 32)]
    ids1 = text[:8] + [cfg.image_token_id] + text[8:48]                 # system + image + question
    ids2 = ids1 + text[48:]                                            # + answer + the next question
    hash_ms = []
    out = {}
    for cache in (True, False):
        kv = PagedKVCache(cfg.llm.num_layers, m.llm.Hkv, cfg.llm.head_dim, num_blocks=args.kv_blocks, device=dev,
                          dtype=torch.float8_e4m3fn if args.kv_fp8 else torch.bfloat16)

        def build(a):
            ids, img = a
            if isinstance(img, PreparedPrefill):
                return img.x
            if isinstance(img, CachedImagePrefill):
                return m.llm.embed_tokens(h2d_ahead(img.full_ids, dev, torch.long))
            return m.build_prefill(ids, [img])

        eng = LLMEngine(m.llm, kv, build, max_batch=4)

        def one(ids, jpeg):
            t_arrive = time.perf_counter()
            full, starts = m.expand_image_tokens(ids, 1)
            keys = hit = None
            if cache:
                t = time.perf_counter()
                keys = prefix_cache_keys(full, starts, hashlib.blake2b(jpeg, digest_size=16).digest())
                hash_ms.append((time.perf_counter() - t) * 1000)
                hit = eng.match_prefix(keys, len(full))
            if hit is not None and hit.tokens > 0 and all(s + N <= hit.tokens for s in starts):
                img = CachedImagePrefill(full)
            else:
                img = decode_image(jpeg, dev, draft_to=(cfg.vision.image_size, cfg.vision.image_size))
                if ENCODE_AHEAD:
                    pre = m.prepare_prefill(ids, [img])
                    img = pre if pre is not None else img
            r = eng.submit((ids, img), len(full), SamplingParams(max_new_tokens=4), prefix_keys=keys, hit=hit)
            list(r.stream(timeout=600))
            return (r.t_first - t_arrive) * 1000, r.cached_tokens, len(full)

        t1, t2, c2 = [], [], []
        for i, jpeg in enumerate(jpegs):
            a, _, n1 = one(ids1, jpeg)
            b, cached, n2 = one(ids2, jpeg)
            if i >= args.warmup:
                t1.append(a)
                t2.append(b)
                c2.append(cached)
        stats = dict(eng.stats)
        eng.close()
        del kv
        tag = "cache_on" if cache else "cache_off"
        out[tag] = {"turn1_ttft_ms_p50": float(np.median(t1)), "turn2_ttft_ms_p50": float(np.median(t2)),
                    "turn1_ttft_ms_min": float(np.min(t1)), "turn2_ttft_ms_min": float(np.min(t2)),
                    "turn1_rows": n1, "turn2_rows": n2, "turn2_cached_tokens": int(np.median(c2)),
                    "turn2_over_turn1": float(np.median(t2) / np.median(t1)), "prefix_hits": stats["prefix_hits"],
                    "prefill_tokens": stats["prefill_tokens"]}
    out.update({"what": "TTFT turn 1 (new image) vs turn 2 (same image, one more user turn)", "preset": args.preset,
                "weights": "bf16" if args.bf16 else "fp8", "kv": "fp8" if args.kv_fp8 else "bf16", "n": args.n,
                "jpeg_kib": len(jpegs[0]) // 1024, "hash_and_keys_ms_p50": float(np.median(hash_ms)),
                "hash_and_keys_ms_max": float(np.max(hash_ms))})
    print(json.dumps(out), flush=True)
    return out


def rows_sweep(args) -> dict:
    """Decoder-only time of a warm prefill by row count: T new rows at position 576 over a cached
    576-token prefix (what a prefix hit leaves to compute), against the cold 624-row prefill."""
    dev = torch.device("cuda")
    cfg = VLM_PRESETS[args.preset]
    m = VLM(cfg, device=dev)
    m.random_init(0)
    if not args.bf16:
        m.quantize_fp8()
    llm = m.llm
    kv = PagedKVCache(cfg.llm.num_layers, llm.Hkv, cfg.llm.head_dim, num_blocks=64, device=dev,
                      dtype=torch.float8_e4m3fn if args.kv_fp8 else torch.bfloat16)
    assert kv.blocks.reserve(1, 1280)
    ids = torch.randint(1000, 30000, (1280,), device=dev)
    tab = torch.from_numpy(np.asarray(kv.blocks.table(1), np.int64)).to(dev)

    def run(start, T):
        x = llm.embed_tokens(ids[start:start + T])
        slots = torch.from_numpy(kv.slots(1, start, T)).to(dev)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        llm.prefill(x, kv, slots, start_pos=start, prefix_blocks=tab[:-(-(start + T) // 64)] if start else None)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    out = {"what": "LLM.prefill device time by rows (start_pos 576 unless cold)", "preset": args.preset,
           "weights": "bf16" if args.bf16 else "fp8"}
    for name, start, T in [("cold_624", 0, 624)] + [(f"warm_{t}", 576, t) for t in (16, 32, 48, 96, 192, 384)]:
        ts = [run(start, T) for _ in range(12)][2:]
        out[name + "_ms"] = float(np.median(ts))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="llava-llama3-8b")
    ap.add_argument("--bf16", action="store_true", help="bf16 decoder weights instead of fp8")
    ap.add_argument("--kv-fp8", action="store_true")
    ap.add_argument("--n", type=int, default=10, help="conversations (one new image each) per cache setting")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kv-blocks", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=40, help="timed calls per path and shape in the kernel comparison")
    ap.add_argument("--shapes", default="", help="start_pos:T,... for the kernel comparison (default: the four recorded shapes)")
    ap.add_argument("--skip-ttft", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--rows-sweep", action="store_true", help="also time LLM.prefill alone by number of new rows")
    args = ap.parse_args()
    load_hip(required=True)
    if not args.skip_kernel:
        shapes = tuple(tuple(int(v) for v in p.split(":")) for p in args.shapes.split(",") if p) or SHAPES
        kernel_bench(args.iters, shapes)
    if not args.skip_ttft:
        ttft_bench(args)
    if args.rows_sweep:
        rows_sweep(args)


if __name__ == "__main__":
    main()
