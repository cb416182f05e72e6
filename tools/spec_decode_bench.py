#!/usr/bin/env python
"""What speculative decoding costs and gains (random weights; needs a GPU).

Three measurements, each in interleaved windows (all variants inside every repetition, medians
reported), for bf16 and fp8 weights of one model preset:

1. step time at B = 1 of the captured decode graph against the captured verify graph at
   T = 2, 4, 8 rows, context about 650 tokens: launch + replay + result read-back, host clock
   around a window of steps that ends in the read-back's wait;
2. the attention kernels alone, per layer: ``paged_decode`` (with and without the fused RoPE)
   against ``rope_kv + paged_verify`` at the same T, device events around a window of launches;
3. the engine end to end with the n-gram drafter off and on over a few synthetic prompts (their
   construction is printed): tok/s after the first token, verify steps and acceptance rate.  The
   weights are random, so the "text" is whatever a random model repeats -- the acceptance rates
   say how the machinery behaves on repetitive and non-repetitive token streams, not what a
   trained model would reach on real text.  A random model's arg-max is a near-tie at many
   positions (top-2 gaps below the bf16 rounding of the logits), and a verify step rounds
   differently from a decode step (separate RoPE launch, other GEMM row counts), so over 128
   tokens the two runs usually part at some position; the line says where.  Exact equality is
   what tests/test_spec_decode_gpu.py asserts.

    python tools/spec_decode_bench.py --model llama3-8b --out profiles/spec_decode_v1.txt

``--sampled``: the same questions for sampled and penalised requests (temperature 0.8, top-p 0.9,
repetition penalty 1.1; ``LUMEN_SPEC_SAMPLING``), bf16 weights:

1. step time of the captured ``"verify_sample"`` graph against the ``"verify"`` graph at T = 4 rows
   and B = 1, 4, 8 sequences (R = 4, 16, 32 rows), and against the in-graph ``"sample"`` decode step
   at the same B.  With ``--base-tree DIR`` (a built checkout of the comparison base) the
   ``"sample"`` step is also measured there: the tool starts one child process per tree and round,
   base and this tree in turn, so the windows of the two builds interleave on the same box;
2. the engine end to end with the n-gram drafter off and on for such requests.

    python tools/spec_decode_bench.py --sampled --model qwen2-0.5b --base-tree ../base --out profiles/spec_sampling_v1.txt
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

# --tree DIR (child processes of --sampled --base-tree): measure the package of that checkout
_TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv[:-1] else str(Path(__file__).resolve().parents[1])
sys.path.insert(0, _TREE)

from lumen_amd.models.llm import LLM, LLM_PRESETS  # noqa: E402
from lumen_amd.ops import llm as lops  # noqa: E402
from lumen_amd.runtime.engine import DecodeGraphs, LLMEngine, SamplingParams  # noqa: E402
from lumen_amd.runtime.kv_cache import PagedKVCache  # noqa: E402
from lumen_amd.runtime.spec_decode import NgramDrafter  # noqa: E402

DEV = "cuda"
LINES: list = []


def say(s: str = "") -> None:
    print(s, flush=True)
    LINES.append(s)


def med(xs):
    return statistics.median(xs)


def step_times(m, cfg, ctx0: int, Ts, reps: int, steps: int) -> dict:
    """median ms per step of the decode graph and of the verify graph per T (B = 1)"""
    kv = PagedKVCache(cfg.num_layers, m.Hkv, cfg.head_dim, num_blocks=32, device=DEV)
    assert kv.blocks.reserve(1, ctx0 + 64)
    g = DecodeGraphs(m, kv, max_batch=1, max_blocks=-(-cfg.max_position // 64))
    bt = kv.block_table([1])
    rng = np.random.default_rng(0)

    def decode_step():
        h = g.launch(rng.integers(0, cfg.vocab_size, 1), np.array([ctx0], np.int32), kv.slots(1, ctx0, 1), bt,
                     np.array([ctx0 + 1], np.int32))
        return lambda: g.tokens(h)

    def verify_step(T):
        def f():
            h = g.launch_verify(rng.integers(0, cfg.vocab_size, T), ctx0 + np.arange(T, dtype=np.int32),
                                kv.slots(1, ctx0, T), bt, np.array([ctx0 + T], np.int32), np.array([T], np.int32), T)
            return lambda: g.verified(h)
        return f

    variants = {"decode": decode_step, **{f"verify T={T}": verify_step(T) for T in Ts}}
    out = {k: [] for k in variants}
    for rep in range(reps + 1):                        # repetition 0 captures and warms up
        for name, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                f()()
            dt = (time.perf_counter() - t0) / steps * 1e3
            if rep:
                out[name].append(dt)
    return {k: (med(v), min(v), max(v)) for k, v in out.items()}


def kernel_times(cfg, m, ctx0: int, Ts, reps: int, iters: int, dtype) -> dict:
    """median us per launch: paged_decode (unfused / fused RoPE) vs rope_kv + paged_verify, one layer"""
    H, Hkv, D = m.H, m.Hkv, cfg.head_dim
    nb = -(-(ctx0 + 8) // 64)
    g = torch.Generator(device=DEV).manual_seed(1)
    kc = torch.randn((nb + 2, Hkv, 64, D), device=DEV, generator=g).to(dtype)
    vc = torch.randn((nb + 2, Hkv, D, 64), device=DEV, generator=g).to(dtype)
    W = next(b for b in (8, 32, 128) if nb <= b)      # the graphs' block-table width bucket
    bt = torch.zeros((1, W), dtype=torch.int32, device=DEV)
    bt[0, :nb] = torch.randperm(nb + 2, device=DEV)[:nb].int()
    ws: dict = {}

    def rows(T):
        return torch.randn((T, (H + 2 * Hkv) * D), device=DEV, generator=g).bfloat16()

    def mk_decode(fused):
        q = rows(1)
        pos = torch.tensor([ctx0], dtype=torch.int32, device=DEV)
        slot = (bt[0, ctx0 // 64].long() * 64 + ctx0 % 64).view(1)
        ctx = torch.tensor([ctx0 + 1], dtype=torch.int32, device=DEV)

        def f():
            if not fused:
                lops.rope_kv(q, pos, m.cos_sin, H, Hkv, D, slot, kc, vc)
            lops.paged_decode(q, kc, vc, bt, ctx, H, Hkv, workspace=ws, rope=(pos, m.cos_sin, slot) if fused else None)
        return f

    def mk_verify(T):
        q = rows(T)
        pos = (ctx0 + torch.arange(T, device=DEV)).int()
        slots = bt[0, (pos // 64).long()].long() * 64 + (pos % 64).long()
        ctx = torch.tensor([ctx0 + T], dtype=torch.int32, device=DEV)
        n = torch.tensor([T], dtype=torch.int32, device=DEV)

        def f():
            lops.rope_kv(q, pos, m.cos_sin, H, Hkv, D, slots, kc, vc)
            lops.paged_verify(q, kc, vc, bt, ctx, n, T, H, Hkv, workspace=ws)
        return f

    variants = {"paged_decode fused rope": mk_decode(True), "rope_kv + paged_decode": mk_decode(False),
                **{f"rope_kv + paged_verify T={T}": mk_verify(T) for T in Ts}}
    out = {k: [] for k in variants}
    for rep in range(reps + 1):
        for name, f in variants.items():
            for _ in range(5):
                f()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            e1.synchronize()
            if rep:
                out[name].append(e0.elapsed_time(e1) / iters * 1e3)
    return {k: (med(v), min(v), max(v)) for k, v in out.items()}


SAMPLED = dict(temperature=0.8, top_p=0.9, repetition_penalty=1.1)


def sampled_step_windows(m, cfg, ctx0: int, Bs, T: int, reps: int, steps: int, verify: bool) -> dict:
    """ms per step, one value per window, of the captured graphs at B sequences: the ``sample``
    decode step and (``verify``) the ``verify`` and ``verify_sample`` steps of T rows per sequence.
    Every sequence is sampled and penalised; its bitmap slot holds 200 random tokens."""
    Bmax = max(Bs)
    kv = PagedKVCache(cfg.num_layers, m.Hkv, cfg.head_dim, num_blocks=Bmax * (-(-(ctx0 + 64) // 64) + 1), device=DEV)
    for b in range(Bmax):
        assert kv.blocks.reserve(b + 1, ctx0 + 64)
    g = DecodeGraphs(m, kv, max_batch=Bmax, max_blocks=-(-cfg.max_position // 64))
    rng = np.random.default_rng(0)
    slots = [g.take_slot() for _ in range(Bmax)]
    for s in slots:
        g.write_slot(s, rng.integers(0, cfg.vocab_size, 200))

    def smp(B, rows):
        return {"inv_t": np.full(B, 1.0 / SAMPLED["temperature"], np.float32), "top_p": np.full(B, SAMPLED["top_p"]),
                "penalty": np.full(B, SAMPLED["repetition_penalty"], np.float32), "greedy": np.zeros(B, np.int32),
                "seen_slot": np.array(slots[:B], np.int32), "u": rng.random(rows)}

    def decode_step(B):
        rids = list(range(1, B + 1))
        bt = kv.block_table(rids)
        sl = np.concatenate([kv.slots(r, ctx0, 1) for r in rids])

        def f():
            h = g.launch(rng.integers(0, cfg.vocab_size, B), np.full(B, ctx0, np.int32), sl, bt,
                         np.full(B, ctx0 + 1, np.int32), sample=smp(B, B))
            return lambda: g.sampled(h)
        return f

    def verify_step(B, sampled):
        rids = list(range(1, B + 1))
        bt = kv.block_table(rids)
        sl = np.concatenate([kv.slots(r, ctx0, T) for r in rids])
        pos = np.tile(ctx0 + np.arange(T, dtype=np.int32), B)

        def f():
            kw = {"sample": smp(B, B * T)} if sampled else {}
            h = g.launch_verify(rng.integers(0, cfg.vocab_size, B * T), pos, sl, bt, np.full(B, ctx0 + T, np.int32),
                                np.full(B, T, np.int32), T, **kw)
            return lambda: g.verified(h)
        return f

    variants = {}
    for B in Bs:
        variants[f"sample decode B={B}"] = decode_step(B)
        if verify:
            variants[f"verify B={B} T={T}"] = verify_step(B, False)
            variants[f"verify_sample B={B} T={T}"] = verify_step(B, True)
    out = {k: [] for k in variants}
    for rep in range(reps + 1):                        # repetition 0 captures and warms up
        for name, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                f()()
            if rep:
                out[name].append((time.perf_counter() - t0) / steps * 1e3)
    return out


def sampled_child(a, tree: str, verify: bool) -> dict:
    """one child process of this tool on the package of ``tree``: its step windows"""
    cmd = [sys.executable, str(Path(__file__).resolve()), "--sampled-child", "--model", a.model, "--ctx", str(a.ctx),
           "--reps", str(a.reps), "--steps", str(a.steps), "--tree", tree] + ([] if verify else ["--no-verify"])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"child on {tree} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(next(ln for ln in reversed(r.stdout.splitlines()) if ln.startswith("{")))


def sampled_main(a) -> None:
    cfg = LLM_PRESETS[a.model]
    Bs, T = (1, 4, 8), 4
    if a.sampled_child:
        m = LLM(cfg, device=DEV)
        m.random_init(1)
        print(json.dumps(sampled_step_windows(m, cfg, a.ctx, Bs, T, a.reps, a.steps, not a.no_verify)), flush=True)
        return
    say(f"# speculative decoding of sampled / penalised requests: {a.model}, random weights, bf16, "
        f"{torch.cuda.get_device_name(0)}")
    say(f"# every request: temperature {SAMPLED['temperature']}, top-p {SAMPLED['top_p']}, repetition penalty "
        f"{SAMPLED['repetition_penalty']}; context {a.ctx}, T = {T} rows per sequence")
    here = str(Path(__file__).resolve().parents[1])
    win: dict = {}
    base: dict = {}
    for _ in range(a.rounds):                          # base and this tree in turn: their windows interleave
        if a.base_tree:
            for k, v in sampled_child(a, a.base_tree, False).items():
                base.setdefault(k, []).extend(v)
        for k, v in sampled_child(a, here, True).items():
            win.setdefault(k, []).extend(v)
    n = len(next(iter(win.values())))
    say()
    say(f"step time, captured graphs: launch + replay + read-back, {a.steps} steps per window, medians (min .. max) of "
        f"{n} windows in {a.rounds} processes per tree (ms)")
    for B in Bs:
        v, vs, d = (win[f"verify B={B} T={T}"], win[f"verify_sample B={B} T={T}"], win[f"sample decode B={B}"])
        say(f"  B = {B}, R = {B * T} rows")
        say(f"    verify               {med(v):7.3f}  ({min(v):.3f} .. {max(v):.3f})")
        say(f"    verify_sample        {med(vs):7.3f}  ({min(vs):.3f} .. {max(vs):.3f})  x{med(vs) / med(v):.2f} of verify, "
            f"+{(med(vs) - med(v)) * 1e3:.0f} us")
        say(f"    sample decode step   {med(d):7.3f}  ({min(d):.3f} .. {max(d):.3f})  this tree; verify_sample is "
            f"x{med(vs) / med(d):.2f} of it")
        if base:
            p = base[f"sample decode B={B}"]
            say(f"    sample decode step   {med(p):7.3f}  ({min(p):.3f} .. {max(p):.3f})  base tree; verify_sample is "
                f"x{med(vs) / med(p):.2f} of it, this tree's decode step x{med(d) / med(p):.3f}")
    m = LLM(cfg, device=DEV)
    m.random_init(1)
    # the sampled requests of a random model draw from 64 near-equal candidates, so their output never
    # repeats and the n-gram drafter finds nothing to propose; the penalised greedy requests show the
    # sampled verify step at work on streams that do repeat
    for what, params in (("sampled + penalised requests, seed 1", dict(SAMPLED, seed=1)),
                         ("greedy requests with the repetition penalty alone",
                          dict(repetition_penalty=SAMPLED["repetition_penalty"]))):
        say()
        say(f"engine (this tree, LUMEN_SPEC_SAMPLING on), {what}: n-gram drafter off / on, {a.new} new tokens, "
            f"{a.spec_tokens} draft tokens per step (tok/s after the first token)")
        for text, off, on, s, first, distinct in engine_runs(m, cfg, a.new, max(2, a.reps // 2), a.spec_tokens, params):
            acc = s["spec_accepted"] / s["spec_drafted"] if s["spec_drafted"] else float("nan")
            say(f"  prompt {text}")
            say(f"    off {off:7.1f} tok/s   on {on:7.1f} tok/s  x{on / off:.2f}   verify steps {s['spec_steps']} "
                f"({s['spec_sample_steps']} sampled), plain steps {s['decode_steps']}, accepted "
                f"{s['spec_accepted']}/{s['spec_drafted']} = {acc:.2f}, first token differing from the run without "
                f"speculation: {first}, distinct output tokens: {distinct}")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(LINES) + "\n")


def prompts(cfg) -> dict:
    r = np.random.default_rng(7)
    V = cfg.vocab_size
    phrase = [int(t) for t in r.integers(0, V, 16)]
    items = [[int(t) for t in r.integers(0, V, 5)] for _ in range(8)]
    sep = [int(t) for t in r.integers(0, V, 2)]
    lst = [t for i in range(40) for t in sep + items[i % 8]]
    return {"repeat: one 16-token phrase of random ids, 24 times (384 tokens)": phrase * 24,
            "list: 40 entries '2-token separator + one of 8 five-token items' in rotation (280 tokens)": lst,
            "random: 400 independent random ids, nothing repeats": [int(t) for t in r.integers(0, V, 400)]}


def engine_runs(m, cfg, new: int, reps: int, spec_tokens: int, params: dict | None = None) -> list:
    """``params``: SamplingParams fields of every request (sampled / penalised requests: the engine
    then runs with ``spec_sampling`` on)"""
    kw = {"spec_sampling": True} if params else {}
    params = params or {}
    rows = []
    for text, p in prompts(cfg).items():
        res = {False: [], True: []}
        stats = {}
        for rep in range(reps + 1):
            for on in (False, True):
                kv = PagedKVCache(cfg.num_layers, m.Hkv, cfg.head_dim, num_blocks=64, device=DEV)
                eng = LLMEngine(m, kv, lambda ids: m.embed_tokens(torch.tensor(ids, device=DEV)), max_batch=1,
                                use_graphs=True, drafter=NgramDrafter() if on else None, spec_tokens=spec_tokens,
                                **kw)
                try:
                    # the same request once before the timed one: its graphs are captured by then
                    w = eng.submit(p, len(p), SamplingParams(max_new_tokens=new, **params), prompt_ids=p)
                    list(w.stream(timeout=300))
                    base = dict(eng.stats)
                    r = eng.submit(p, len(p), SamplingParams(max_new_tokens=new, **params), prompt_ids=p)
                    list(r.stream(timeout=300))
                    if rep:
                        res[on].append((len(r.tokens) - 1) / (r.t_done - r.t_first))
                    stats[on] = ({k: eng.stats[k] - base.get(k, 0) for k in eng.stats}, list(r.tokens))
                finally:
                    eng.close()
        a, b = stats[False][1], stats[True][1]
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
        rows.append((text, med(res[False]), med(res[True]), stats[True][0], first, len(set(a))))
    return rows


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b", choices=sorted(LLM_PRESETS))
    ap.add_argument("--ctx", type=int, default=650)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--spec-tokens", type=int, default=3)
    ap.add_argument("--weights", default="bf16,fp8")
    ap.add_argument("--out", default=None)
    ap.add_argument("--sampled", action="store_true", help="sampled / penalised requests (LUMEN_SPEC_SAMPLING)")
    ap.add_argument("--base-tree", default=None, help="--sampled: a built checkout of the comparison base")
    ap.add_argument("--rounds", type=int, default=2, help="--sampled: child processes per tree")
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--sampled-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-verify", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spec_decode_bench needs a GPU")
    if a.sampled or a.sampled_child:
        sampled_main(a)
        return
    cfg = LLM_PRESETS[a.model]
    Ts = (2, 4, 8)
    say(f"# speculative decoding: {a.model}, random weights, {torch.cuda.get_device_name(0)}")
    say(f"# B = 1, context {a.ctx}; medians (min .. max) of {a.reps} interleaved windows")
    for wd in a.weights.split(","):
        m = LLM(cfg, device=DEV)
        m.random_init(1)
        if wd == "fp8":
            m.quantize_fp8()
        say()
        say(f"## weights {wd}")
        st = step_times(m, cfg, a.ctx, Ts, a.reps, a.steps)
        d = st["decode"][0]
        say(f"step time, captured graphs, {a.steps} steps per window (ms; ratio to the decode step)")
        for k, (md, lo, hi) in st.items():
            say(f"  {k:<14} {md:7.3f}  ({lo:.3f} .. {hi:.3f})  x{md / d:.2f}")
        for kvd, name in ((torch.bfloat16, "bf16"), (torch.float8_e4m3fn, "fp8")):
            kt = kernel_times(cfg, m, a.ctx, Ts, a.reps, 200, kvd)
            d = kt["paged_decode fused rope"][0]
            say(f"attention per layer, {name} cache, 200 launches per window (us; ratio to the fused decode kernel)")
            for k, (md, lo, hi) in kt.items():
                say(f"  {k:<28} {md:7.2f}  ({lo:.2f} .. {hi:.2f})  x{md / d:.2f}")
        say(f"engine, n-gram drafter off / on, {a.new} new tokens, {a.spec_tokens} draft tokens per step (tok/s after the first token)")
        for text, off, on, s, first, distinct in engine_runs(m, cfg, a.new, max(2, a.reps // 2), a.spec_tokens):
            acc = s["spec_accepted"] / s["spec_drafted"] if s["spec_drafted"] else float("nan")
            say(f"  prompt {text}")
            say(f"    off {off:7.1f} tok/s   on {on:7.1f} tok/s  x{on / off:.2f}   verify steps {s['spec_steps']}, "
                f"plain steps {s['decode_steps']}, accepted {s['spec_accepted']}/{s['spec_drafted']} = {acc:.2f}, "
                f"first token differing from the run without speculation: {first}, distinct output tokens: {distinct}")
        del m
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
