"""Guided decoding: what the ``guided`` decode graph costs next to the ``sample`` graph, whether
look-ahead stays on, and how long three grammars take to compile for a vocabulary of real size.

    python tools/guided_bench.py [--out profiles/guided_v1.txt] [--batches 1,8,32] [--windows 10] [--steps 100]

qwen2-0.5b preset, random weights, a synthetic byte-level vocabulary of 151,936 tokens.

Step time: captured graphs, look-ahead form (the token ids and, in the guided graph, the grammar
states stay on the device), ``--steps`` replays per window ending in a synchronise; windows of the
two graphs alternate, the report gives the median (min .. max) over ``--windows``.  The ``sample``
graph's kernels are instruction for instruction the parent commit's (the guided form is a template
flag).  Every row is sampled (temperature 0.8, top-p 0.9) and, in the guided graph, constrained by
``([a-z]+ )*[a-z]+``, a grammar that never forces the end.

Engine: eight requests of 64 tokens through ``LLMEngine``, unguided sampled against guided, with the
engine's counters (guided steps, look-ahead steps)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lumen_amd.runtime import guided as gd  # noqa: E402

V = 151936
EOS = V - 1
PHOTO_SCHEMA = {"type": "object",
                "properties": {"caption": {"type": "string", "maxLength": 40},
                               "tags": {"type": "array", "items": {"type": "string", "maxLength": 12}, "maxItems": 5},
                               "nsfw": {"type": "boolean"},
                               "people": {"type": "integer"}}}
GRAMMARS = [("choice", ["indoor", "outdoor", "portrait", "landscape", "unclear"], "5-way choice"),
            ("regex", r"\d{4}-\d{2}-\d{2}", r"\d{4}-\d{2}-\d{2}"),
            ("json_schema", PHOTO_SCHEMA, "photo-tag schema (caption <= 40, <= 5 tags <= 12, boolean, integer)")]


def synthetic_vocab(seed: int = 0) -> list:
    """151,936 byte strings shaped like a byte-level BPE vocabulary: the 256 bytes, then words of 2
    to 12 bytes (half of them with a leading space; letters, digits, punctuation, some UTF-8), the
    last 64 ids special (no bytes)"""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"etaoinshrdlucmfwypvbgkqjxzETAOINSHRDLU0123456789.,:;\"'{}[]()-_/\\\n", np.uint8)
    out = [bytes([i]) for i in range(256)]
    n = V - 64 - 256
    lens = rng.integers(2, 13, n)
    lead = rng.random(n) < 0.5
    body = alpha[rng.integers(0, len(alpha), int(lens.sum()))].tobytes()
    at = 0
    for k in range(n):
        w = body[at:at + lens[k]]
        at += lens[k]
        if k % 97 == 0:
            w = "é日ü".encode()[: 2 + k % 5] if k % 2 else "語".encode()
        out.append((b" " if lead[k] else b"") + w)
    return out + [b""] * 64


def compile_times(vocab, lines):
    lines.append("grammar compile, vocabulary of 151,936 tokens (host, one thread): regex -> minimised DFA, then the token tables")
    for kind, spec, name in GRAMMARS:
        t0 = time.perf_counter()
        text = gd.lower(kind, spec)
        dfa, accept = gd.compile_regex(text)
        t1 = time.perf_counter()
        g = gd.compile_guide(kind, spec, vocab, [EOS])
        t2 = time.perf_counter()
        lines.append(f"  {name}: {dfa.shape[0]} states; DFA {1e3 * (t1 - t0):.0f} ms, whole guide {1e3 * (t2 - t1):.0f} ms, "
                     f"tables {g.allow.nbytes / 1e6:.1f} MB")
    lines.append("")


def step_times(args, vocab, lines):
    import torch

    from lumen_amd.models.llm import LLM, LLM_PRESETS
    from lumen_amd.runtime.engine import DecodeGraphs, GuideArena
    from lumen_amd.runtime.kv_cache import PagedKVCache

    cfg = LLM_PRESETS["qwen2-0.5b"]
    m = LLM(cfg, device="cuda")
    m.random_init(5)
    batches = [int(b) for b in args.batches.split(",")]
    ctx0 = 256
    kv = PagedKVCache(cfg.num_layers, m.Hkv, cfg.head_dim, num_blocks=max(batches) * 6 + 8, device="cuda")
    graphs = DecodeGraphs(m, kv, max(batches), -(-cfg.max_position // 64))
    guide = gd.compile_guide("regex", r"([a-z]+ )*[a-z]+", vocab, [EOS])
    arena = GuideArena(m, max(batches), vocab)
    graphs.arena = arena
    base = arena.acquire(guide)
    lines.append(f"decode step, captured graphs, look-ahead form, context {ctx0}: {args.steps} replays per window, "
                 f"median (min .. max) of {args.windows} alternating windows (ms per step)")
    for B in batches:
        for b in range(B):
            kv.blocks.reserve(1000 + b, ctx0 + 64)
        rids = [1000 + b for b in range(B)]
        pos = np.full(B, ctx0, np.int32)
        slots = np.concatenate([kv.slots(r, ctx0, 1) for r in rids])
        bt = kv.block_table(rids)
        rng = np.random.default_rng(B)

        def sample(guided, fed):
            s = {"inv_t": np.full(B, 1 / 0.8, np.float32), "top_p": np.full(B, 0.9), "penalty": np.ones(B, np.float32),
                 "greedy": np.zeros(B, np.int32), "seen_slot": np.full(B, -1, np.int32), "u": rng.random(B)}
            if guided:
                s["g_slot"] = np.arange(B, dtype=np.int32)
                s["g_in"] = np.full(B, base + guide.start if fed else -1, np.int32)
            return s

        def window(guided):
            h = graphs.launch(np.full(B, 97, np.int64), pos, slots, bt, pos + 1, sample=sample(guided, True))
            graphs.sampled(h)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                h = graphs.launch(None, pos, slots, bt, pos + 1, sample=sample(guided, False))
            toks = graphs.sampled(h)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / args.steps
            assert (toks >= 0).all()
            return 1e3 * dt

        for g in (False, True):       # capture + warm both graphs
            window(g)
        res = {False: [], True: []}
        for _ in range(args.windows):
            for g in (False, True):
                res[g].append(window(g))
        f = lambda x: f"{statistics.median(x):.3f} ({min(x):.3f} .. {max(x):.3f})"  # noqa: E731
        ms, mg = statistics.median(res[False]), statistics.median(res[True])
        lines.append(f"  B = {B:2d}: sample {f(res[False])}   guided {f(res[True])}   guided - sample = "
                     f"{1e3 * (mg - ms):+.1f} us, x{mg / ms:.3f}")
        for r in rids:
            kv.blocks.release(r)
    lines.append("")
    return m


def engine_run(m, vocab, lines):
    import torch

    from lumen_amd.models.llm import LLM_PRESETS
    from lumen_amd.runtime.engine import LLMEngine, SamplingParams
    from lumen_amd.runtime.kv_cache import PagedKVCache

    cfg = LLM_PRESETS["qwen2-0.5b"]
    guide = gd.compile_guide("regex", r"([a-z]+ )*[a-z]+", vocab, [EOS])
    prompts = [list(np.random.default_rng(i).integers(0, 150000, 48)) for i in range(8)]
    lines.append("engine, 8 requests x 64 tokens, temperature 0.8, top-p 0.9 (tok/s over the whole run, 3 runs each, in turn)")
    kv = PagedKVCache(cfg.num_layers, m.Hkv, cfg.head_dim, num_blocks=64, device="cuda")
    eng = LLMEngine(m, kv, lambda ids: m.embed_tokens(torch.tensor(ids, device="cuda")), max_batch=8)
    try:
        def run(guided):
            t0 = time.perf_counter()
            rs = [eng.submit(p, len(p), SamplingParams(max_new_tokens=64, temperature=0.8, top_p=0.9, seed=i,
                                                       stop_token_ids=(EOS,), guide=guide if guided else None))
                  for i, p in enumerate(prompts)]
            for r in rs:
                list(r.stream(timeout=300))
            return sum(len(r.tokens) for r in rs) / (time.perf_counter() - t0)

        run(False), run(True)          # captures
        before = dict(eng.stats)
        rates = {False: [], True: []}
        for _ in range(3):
            for g in (False, True):
                rates[g].append(run(g))
        st = {k: eng.stats.get(k, 0) - before.get(k, 0) for k in ("guided_steps", "ingraph_sample_steps",
                                                                   "lookahead_steps", "decode_steps")}
    finally:
        eng.close()
    for g in (False, True):
        lines.append(f"  {'guided  ' if g else 'unguided'}: {statistics.median(rates[g]):.0f} tok/s "
                     f"({min(rates[g]):.0f} .. {max(rates[g]):.0f})")
    lines.append(f"  counters over the six timed runs: {json.dumps(st)}")
    lines.append(f"  look-ahead stayed on: {'yes' if st['guided_steps'] > 0 and st['lookahead_steps'] > 0 else 'NO'} "
                 f"({st['lookahead_steps']} of {st['decode_steps']} decode steps were launched one step ahead)")
    lines.append("")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/guided_v1.txt")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--compile-only", action="store_true", help="grammar compile times only (no GPU needed)")
    args = ap.parse_args()
    vocab = synthetic_vocab()
    lines = []
    if not args.compile_only:
        import torch

        if not torch.cuda.is_available():
            raise SystemExit("guided_bench: the step times need a GPU (--compile-only runs without)")
        lines.append(f"# guided decoding: qwen2-0.5b, random weights, bf16, V = {V}, {torch.cuda.get_device_name(0)}")
        lines.append("")
        m = step_times(args, vocab, lines)
        engine_run(m, vocab, lines)
    compile_times(vocab, lines)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
