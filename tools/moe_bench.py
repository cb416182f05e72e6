#!/usr/bin/env python
"""Time the sparse MoE MLP (ops.llm.moe_mlp, csrc/moe.hip) at the Qwen3-30B-A3B layer shape against
the dense MLP that reads the same weight bytes at T = 1.

    python tools/moe_bench.py [--layers 8] [--iters 50] [--rows 1,8,32,512,2048]

Per row count T it reports, per layer call: the time of moe_mlp (route + group + two grouped GEMMs
+ combine), the time of the dense equivalent on the existing ops -- a gate|up + down pair of
intermediate size k * I through ops.linear_dec (T <= 32) / ops.linear -- the expert-weight bytes
the routing touched (distinct experts x 3 I H x 2 bytes, counted from the ids) per second, and the
ratio of the two times.

How the numbers are taken: both chains are captured into a graph on a private stream (decode runs
from graphs; an eager call would time the host's launches) that walks ``--layers`` independent
weight sets, so no layer finds its weights in the 256 MB Infinity Cache from the previous replay
(8 experts x 9.4 MB x 8 layers at T = 1); every shape is warmed up; device events bracket
``--iters`` replays; the two chains alternate over 5 rounds and the median and the minimum are
printed.  One JSON line per row count, then a table.  Needs a GPU: there is no CPU fall-back.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lumen_amd import ops  # noqa: E402
from lumen_amd.models.llm import LLM_PRESETS  # noqa: E402
from lumen_amd.ops import llm as lops  # noqa: E402


def _rand(shape, std, gen, dev):
    out = torch.empty(shape, device=dev, dtype=torch.bfloat16)
    flat = out.view(-1)
    step = 1 << 26                                          # bounded fp32 temporaries
    for i in range(0, flat.numel(), step):
        n = min(step, flat.numel() - i)
        flat[i:i + n] = (torch.randn(n, generator=gen, device=dev, dtype=torch.float32) * std).bfloat16()
    return out


def _graph(run, stream):
    """Warm ``run`` up twice on ``stream``, capture it there, return the graph."""
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run()
        run()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.CAPTURE_LOCK, torch.cuda.graph(g, stream=stream):
        run()
    return g


def _time(g, iters):
    """ms per replay: device events around ``iters`` replays"""
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=8, help="independent weight sets walked per replay")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", default="1,8,32,512,2048")
    ap.add_argument("--preset", default="qwen3-30b-a3b")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moe_bench: no GPU (the timings are GPU measurements; there is no CPU fall-back)")
    dev = torch.device("cuda", 0)
    cfg = LLM_PRESETS[args.preset]
    H, I, E, k = cfg.hidden_size, cfg.moe_intermediate_size, cfg.num_experts, cfg.num_experts_per_tok
    L = args.layers
    gen = torch.Generator(device=dev).manual_seed(0)
    moe = [dict(gate=_rand((E, H), H ** -0.5, gen, dev), gu=_rand((E, 2 * I, H), H ** -0.5, gen, dev),
                down=_rand((E, H, I), I ** -0.5, gen, dev)) for _ in range(L)]
    Id = k * I                                               # the dense MLP of the same active bytes
    dense = [dict(gu=_rand((2 * Id, H), H ** -0.5, gen, dev), down=_rand((H, Id), Id ** -0.5, gen, dev))
             for _ in range(L)]
    stream = ops.private_stream(dev)
    rows_out = []
    for T in [int(t) for t in args.rows.split(",")]:
        xs = [_rand((T, H), 1.0, gen, dev) for _ in range(L)]
        outs = [torch.empty_like(x) for x in xs]

        def run_moe():
            for l in range(L):
                lops.moe_mlp(xs[l], moe[l]["gate"], moe[l]["gu"], moe[l]["down"], k, residual=xs[l], out=outs[l])

        def run_dense():
            for l in range(L):
                if T <= 32:
                    g = ops.linear_dec(xs[l], dense[l]["gu"], glu=True)
                    ops.linear_dec(g, dense[l]["down"], residual=xs[l], out=outs[l])
                else:
                    g = ops.linear(xs[l], dense[l]["gu"], glu=True)
                    ops.linear(g, dense[l]["down"], residual=xs[l], out=outs[l])

        touched = 0                                          # expert-weight bytes the routing reads, all layers
        for l in range(L):
            ids, _ = lops.moe_route(xs[l], moe[l]["gate"], k)
            touched += int(torch.unique(ids).numel()) * 3 * I * H * 2
        gm, gd = _graph(run_moe, stream), _graph(run_dense, stream)
        tm, td = [], []
        for _ in range(args.rounds):                         # alternate the two chains
            tm.append(_time(gm, args.iters) / L)
            td.append(_time(gd, args.iters) / L)
        m_med, d_med = statistics.median(tm), statistics.median(td)
        rec = dict(T=T, E=E, k=k, H=H, I=I, layers=L, iters=args.iters,
                   moe_us=round(m_med * 1e3, 2), moe_us_min=round(min(tm) * 1e3, 2),
                   dense_us=round(d_med * 1e3, 2), dense_us_min=round(min(td) * 1e3, 2),
                   expert_bytes_per_layer=touched // L,
                   expert_GBps=round(touched / L / (m_med * 1e-3) / 1e9, 1),
                   dense_bytes_per_layer=3 * Id * H * 2,
                   dense_GBps=round(3 * Id * H * 2 / (d_med * 1e-3) / 1e9, 1),
                   moe_over_dense=round(m_med / d_med, 3))
        rows_out.append(rec)
        print(json.dumps(rec), flush=True)
        del gm, gd
    print(f"\n{args.preset} layer: H {H}, I {I}, E {E}, k {k}; per layer call, median of {args.rounds} rounds x "
          f"{args.iters} graph replays over {L} weight sets")
    print(f"{'T':>6} {'moe us':>10} {'dense us':>10} {'moe/dense':>10} {'experts MB':>11} {'expert GB/s':>12} {'dense GB/s':>11}")
    for r in rows_out:
        print(f"{r['T']:>6} {r['moe_us']:>10.1f} {r['dense_us']:>10.1f} {r['moe_over_dense']:>10.2f} "
              f"{r['expert_bytes_per_layer'] / 1e6:>11.1f} {r['expert_GBps']:>12.1f} {r['dense_GBps']:>11.1f}")


if __name__ == "__main__":
    main()
