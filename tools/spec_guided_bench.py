"""Speculative decoding of guided requests (``LUMEN_SPEC_GUIDED``): the same guided engine job with
``spec_guided`` off and on, and what the ``verify_guided`` graph costs next to ``verify_sample``.

    python tools/spec_guided_bench.py [--out profiles/spec_guided_v1.txt] [--batches 1,8] [--runs 5] [--steps 100]

qwen2-0.5b preset, random weights, bf16, the synthetic byte-level vocabulary of 151,936 tokens of
tools/guided_bench.py, its four-property photo-tag schema and a short regex.

Engine: B greedy requests under one grammar, three engines over one model in one process: ``off``
(``spec_guided`` off -- the behaviour before the switch existed: a guided batch takes no verify
steps), ``forced`` (the switch alone: the grammar's forced tokens are the only draft) and
``forced+ngram`` (the switch and the n-gram drafter).  The timed runs alternate between the engines;
tok/s counts the tokens after the first of every request over the time from the first token of the
last request to the end.  The counters are those of the timed runs.

Step: captured graphs at the same (B, T = 4), every row live and sampled (temperature 0.8, top-p
0.9), ``--steps`` replays per window, windows of the two graphs alternating; in the guided graph
every row draws in the start state of ``([a-z]+ )*[a-z]+``."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from guided_bench import EOS, PHOTO_SCHEMA, V, synthetic_vocab  # noqa: E402
from lumen_amd.runtime import guided as gd  # noqa: E402

JOBS = [("json_schema", PHOTO_SCHEMA, "photo-tag schema", 96), ("regex", r"\d{4}-\d{2}-\d{2}", r"\d{4}-\d{2}-\d{2}", 16)]
COUNTERS = ("decode_steps", "spec_steps", "spec_guided_steps", "spec_drafted", "spec_accepted", "spec_forced_drafted",
            "spec_forced_accepted", "guided_steps", "tokens")
T = 4


def engine_runs(m, vocab, batches, runs, lines):
    import torch

    from lumen_amd.models.llm import LLM_PRESETS
    from lumen_amd.runtime.engine import LLMEngine, SamplingParams
    from lumen_amd.runtime.kv_cache import PagedKVCache
    from lumen_amd.runtime.spec_decode import NgramDrafter

    cfg = LLM_PRESETS["qwen2-0.5b"]
    Bmax = max(batches)
    prompts = [[int(t) for t in np.random.default_rng(i).integers(0, 150000, 48)] for i in range(Bmax)]
    kinds = {"off": dict(spec_guided=False), "forced": dict(spec_guided=True),
             "forced+ngram": dict(spec_guided=True, drafter=NgramDrafter())}
    engines = {}
    for name, kw in kinds.items():
        kv = PagedKVCache(cfg.num_layers, m.Hkv, cfg.head_dim, num_blocks=Bmax * 4 + 8, device="cuda")
        engines[name] = LLMEngine(m, kv, lambda ids: m.embed_tokens(torch.tensor(ids, device="cuda")), max_batch=Bmax,
                                  spec_tokens=T - 1, **kw)
    try:
        for kind, spec, title, new in JOBS:
            guide = gd.compile_guide(kind, spec, vocab, [EOS])
            lines.append(f"engine, greedy requests under the {title} ({guide.n_states} states), at most {new} new tokens, "
                         f"{T - 1} draft tokens per step (tok/s after the first token; median (min .. max) of {runs} "
                         "runs, the engines in turn)")
            for B in batches:
                def run(eng):
                    hold, eng.max_prefill = eng.max_prefill, 0          # every request joins in the same iteration
                    rs = [eng.submit(p, len(p), SamplingParams(max_new_tokens=new, stop_token_ids=(EOS,), guide=guide),
                                     prompt_ids=p) for p in prompts[:B]]
                    eng.max_prefill = max(hold, B)
                    for r in rs:
                        list(r.stream(timeout=300))
                    eng.max_prefill = hold
                    t0 = max(r.t_first for r in rs)
                    return (sum(len(r.tokens) - 1 for r in rs) / (max(r.t_done for r in rs) - t0),
                            [list(r.tokens) for r in rs], [r.finish_reason for r in rs])

                for eng in engines.values():          # captures, guide upload
                    run(eng)
                before = {n: dict(e.stats) for n, e in engines.items()}
                rates = {n: [] for n in engines}
                toks = {}
                for _ in range(runs):
                    for n, eng in engines.items():
                        rate, toks[n], why = run(eng)
                        rates[n].append(rate)
                base = statistics.median(rates["off"])
                lines.append(f"  B = {B}: {sum(map(len, toks['off']))} tokens, finish reasons {sorted(set(why))}")
                for n, eng in engines.items():
                    st = {k: eng.stats.get(k, 0) - before[n].get(k, 0) for k in COUNTERS}
                    same = sum(a == b for a, b in zip(toks[n], toks["off"]))
                    ng = (st["spec_accepted"] - st["spec_forced_accepted"], st["spec_drafted"] - st["spec_forced_drafted"])
                    r = rates[n]
                    lines.append(f"    {n:13s}: {statistics.median(r):7.0f} tok/s ({min(r):.0f} .. {max(r):.0f})  "
                                 f"x{statistics.median(r) / base:.3f} of off;  steps: {st['spec_guided_steps']} verify + "
                                 f"{st['decode_steps']} decode for {st['tokens']} tokens;  forced accepted "
                                 f"{st['spec_forced_accepted']}/{st['spec_forced_drafted']}, n-gram accepted {ng[0]}/{ng[1]};  "
                                 f"{same}/{B} requests with the tokens of off")
            lines.append("")
    finally:
        for eng in engines.values():
            eng.close()


def step_times(m, vocab, batches, steps, windows, lines):
    import torch

    from lumen_amd.models.llm import LLM_PRESETS
    from lumen_amd.runtime.engine import DecodeGraphs, GuideArena
    from lumen_amd.runtime.kv_cache import PagedKVCache

    cfg = LLM_PRESETS["qwen2-0.5b"]
    ctx0, Bmax = 256, max(batches)
    kv = PagedKVCache(cfg.num_layers, m.Hkv, cfg.head_dim, num_blocks=Bmax * 6 + 8, device="cuda")
    graphs = DecodeGraphs(m, kv, Bmax, -(-cfg.max_position // 64))
    guide = gd.compile_guide("regex", r"([a-z]+ )*[a-z]+", vocab, [EOS])
    arena = GuideArena(m, Bmax, vocab)
    graphs.arena = arena
    base = arena.acquire(guide)
    rng = np.random.default_rng(0)
    lines.append(f"verify step, captured graphs, context {ctx0}, T = {T} live rows per sequence, every row sampled: "
                 f"{steps} replays per window, median (min .. max) of {windows} alternating windows (ms per step)")
    for B in batches:
        rids = [1000 + b for b in range(B)]
        for r in rids:
            assert kv.blocks.reserve(r, ctx0 + 64)
        bt = kv.block_table(rids)
        sl = np.concatenate([kv.slots(r, ctx0, T) for r in rids])
        pos = np.tile(ctx0 + np.arange(T, dtype=np.int32), B)

        def window(guided):
            h = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                s = {"inv_t": np.full(B, 1 / 0.8, np.float32), "top_p": np.full(B, 0.9), "penalty": np.ones(B, np.float32),
                     "greedy": np.zeros(B, np.int32), "seen_slot": np.full(B, -1, np.int32), "u": rng.random(B * T)}
                if guided:
                    s["g_in"] = np.full(B * T, base + guide.start, np.int32)
                h = graphs.launch_verify(rng.integers(97, 123, B * T), pos, sl, bt, np.full(B, ctx0 + T, np.int32),
                                         np.full(B, T, np.int32), T, s)
                toks = graphs.verified(h)
            torch.cuda.synchronize()
            assert (toks[:B * T] >= 0).all()
            return 1e3 * (time.perf_counter() - t0) / steps

        for g in (False, True):       # capture + warm both graphs
            window(g)
        res = {False: [], True: []}
        for _ in range(windows):
            for g in (False, True):
                res[g].append(window(g))
        f = lambda x: f"{statistics.median(x):.3f} ({min(x):.3f} .. {max(x):.3f})"  # noqa: E731
        ms, mg = statistics.median(res[False]), statistics.median(res[True])
        lines.append(f"  B = {B:2d}: verify_sample {f(res[False])}   verify_guided {f(res[True])}   guided - sample = "
                     f"{1e3 * (mg - ms):+.1f} us, x{mg / ms:.3f}")
        for r in rids:
            kv.blocks.release(r)
    lines.append("")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/spec_guided_v1.txt")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    import torch

    from lumen_amd.models.llm import LLM, LLM_PRESETS

    if not torch.cuda.is_available():
        raise SystemExit("spec_guided_bench needs a GPU")
    batches = [int(b) for b in args.batches.split(",")]
    vocab = synthetic_vocab()
    m = LLM(LLM_PRESETS["qwen2-0.5b"], device="cuda")
    m.random_init(5)
    lines = [f"# speculative decoding of guided requests: qwen2-0.5b, random weights, bf16, V = {V}, "
             f"{torch.cuda.get_device_name(0)}", ""]
    engine_runs(m, vocab, batches, args.runs, lines)
    step_times(m, vocab, batches, args.steps, args.windows, lines)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
