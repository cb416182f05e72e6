#!/usr/bin/env python
"""Time the sparse MoE MLP (ops.llm.moe_mlp, csrc/moe.hip, csrc/moe_wq.hip) at the Qwen3-30B-A3B layer
shape against the dense MLP that reads the same weight bytes at T = 1, per expert weight format.

    python tools/moe_bench.py [--layers 8] [--iters 50] [--rows 1,8,32,512,2048] [--weights bf16,fp8,w4]

Per row count T and weight format it reports, per layer call: the time of moe_mlp (route + group + two
grouped GEMMs + combine), the time of the dense equivalent on the existing ops -- a gate|up + down pair
of intermediate size k * I in the same format through ops.linear_dec (T <= 32) / ops.linear -- the
expert bytes the routing touched (distinct experts x the codes and scales / group parameters of one
expert in the format's own bytes, counted from the ids) per second, and the ratio of the two times.
fp8 and 4-bit weights are the bf16 ones quantised (ops.quantize_fp8_rows / ops.quantize_w4_rows), so
every format routes the same way.

How the numbers are taken: every chain is captured into a graph on a private stream (decode runs
from graphs; an eager call would time the host's launches) that walks ``--layers`` independent
weight sets, so no layer finds its weights in the 256 MB Infinity Cache from the previous replay
(8 experts x 9.4 MB x 8 layers at T = 1 in bf16); every shape is warmed up; device events bracket
``--iters`` replays; the chains of all formats alternate inside one run over 5 rounds and the median
and the minimum are printed.  One JSON line per row count and format, then a table.  Needs a GPU: there
is no CPU fall-back.
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


def _quantize(fmt, w):
    """bf16 [.., N, K] -> (codes of the same leading shape, scales / group parameters) or (w, None)"""
    if fmt == "bf16":
        return w, None
    lead, K = w.shape[:-1], w.shape[-1]
    c, s = (ops.quantize_fp8_rows if fmt == "fp8" else ops.quantize_w4_rows)(w.reshape(-1, K))
    return c.view(*lead, -1), s.view(*lead, *s.shape[1:])


def _nbytes(*ts):
    return sum(t.numel() * t.element_size() for t in ts if t is not None)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=8, help="independent weight sets walked per replay")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", default="1,8,32,512,2048")
    ap.add_argument("--preset", default="qwen3-30b-a3b")
    ap.add_argument("--weights", default="bf16", help="expert weight formats, comma separated: bf16, fp8, w4")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moe_bench: no GPU (the timings are GPU measurements; there is no CPU fall-back)")
    fmts = args.weights.split(",")
    if not fmts or any(f not in ("bf16", "fp8", "w4") for f in fmts):
        raise SystemExit(f"moe_bench: --weights takes bf16, fp8 and w4, got {args.weights!r}")
    dev = torch.device("cuda", 0)
    cfg = LLM_PRESETS[args.preset]
    H, I, E, k = cfg.hidden_size, cfg.moe_intermediate_size, cfg.num_experts, cfg.num_experts_per_tok
    L = args.layers
    gen = torch.Generator(device=dev).manual_seed(0)
    Id = k * I                                               # the dense MLP of the same active bytes
    gates, moe, dense = [], {f: [] for f in fmts}, {f: [] for f in fmts}
    for _ in range(L):
        gates.append(_rand((E, H), H ** -0.5, gen, dev))
        gu, down = _rand((E, 2 * I, H), H ** -0.5, gen, dev), _rand((E, H, I), I ** -0.5, gen, dev)
        dgu, ddown = _rand((2 * Id, H), H ** -0.5, gen, dev), _rand((H, Id), Id ** -0.5, gen, dev)
        for f in fmts:
            (gw, gs), (dw, ds) = _quantize(f, gu), _quantize(f, down)
            moe[f].append(dict(gu=gw, down=dw, gu_s=gs, down_s=ds))
            (gw, gs), (dw, ds) = _quantize(f, dgu), _quantize(f, ddown)
            dense[f].append(dict(gu=gw, down=dw, gu_s=gs, down_s=ds))
        del gu, down, dgu, ddown
    per_expert = {f: _nbytes(*moe[f][0].values()) // E for f in fmts}      # codes + scales of one expert
    dense_bytes = {f: _nbytes(*dense[f][0].values()) for f in fmts}
    stream = ops.private_stream(dev)
    rows_out = []
    for T in [int(t) for t in args.rows.split(",")]:
        xs = [_rand((T, H), 1.0, gen, dev) for _ in range(L)]
        outs = [torch.empty_like(x) for x in xs]

        def run_moe(f):
            for l in range(L):
                w = moe[f][l]
                lops.moe_mlp(xs[l], gates[l], w["gu"], w["down"], k, residual=xs[l], out=outs[l], gu_s=w["gu_s"],
                             down_s=w["down_s"])

        def run_dense(f):
            for l in range(L):
                w = dense[f][l]
                if T <= 32:
                    g = ops.linear_dec(xs[l], w["gu"], w["gu_s"], glu=True)
                    ops.linear_dec(g, w["down"], w["down_s"], residual=xs[l], out=outs[l])
                else:
                    g = ops.linear(xs[l], w["gu"], glu=True, w_scale=w["gu_s"])
                    ops.linear(g, w["down"], residual=xs[l], out=outs[l], w_scale=w["down_s"])

        distinct = 0                                         # distinct experts the routing reads, all layers
        for l in range(L):
            ids, _ = lops.moe_route(xs[l], gates[l], k)
            distinct += int(torch.unique(ids).numel())
        graphs = {f: (_graph(lambda f=f: run_moe(f), stream), _graph(lambda f=f: run_dense(f), stream)) for f in fmts}
        tm, td = {f: [] for f in fmts}, {f: [] for f in fmts}
        for _ in range(args.rounds):                         # alternate the chains of every format
            for f in fmts:
                tm[f].append(_time(graphs[f][0], args.iters) / L)
                td[f].append(_time(graphs[f][1], args.iters) / L)
        for f in fmts:
            m_med, d_med = statistics.median(tm[f]), statistics.median(td[f])
            touched = distinct * per_expert[f]
            rec = dict(T=T, weights=f, E=E, k=k, H=H, I=I, layers=L, iters=args.iters,
                       moe_us=round(m_med * 1e3, 2), moe_us_min=round(min(tm[f]) * 1e3, 2),
                       dense_us=round(d_med * 1e3, 2), dense_us_min=round(min(td[f]) * 1e3, 2),
                       expert_bytes_per_layer=touched // L,
                       expert_GBps=round(touched / L / (m_med * 1e-3) / 1e9, 1),
                       dense_bytes_per_layer=dense_bytes[f],
                       dense_GBps=round(dense_bytes[f] / (d_med * 1e-3) / 1e9, 1),
                       moe_over_dense=round(m_med / d_med, 3))
            if f != "bf16" and "bf16" in fmts:
                rec["moe_over_bf16"] = round(m_med / statistics.median(tm["bf16"]), 3)
            rows_out.append(rec)
            print(json.dumps(rec), flush=True)
        del graphs
    print(f"\n{args.preset} layer: H {H}, I {I}, E {E}, k {k}; per layer call, median of {args.rounds} rounds x "
          f"{args.iters} graph replays over {L} weight sets")
    print(f"{'T':>6} {'weights':>8} {'moe us':>10} {'dense us':>10} {'moe/dense':>10} {'moe/bf16':>9} {'experts MB':>11} "
          f"{'expert GB/s':>12} {'dense GB/s':>11}")
    for r in rows_out:
        print(f"{r['T']:>6} {r['weights']:>8} {r['moe_us']:>10.1f} {r['dense_us']:>10.1f} {r['moe_over_dense']:>10.2f} "
              f"{r.get('moe_over_bf16', 1.0):>9.2f} {r['expert_bytes_per_layer'] / 1e6:>11.1f} {r['expert_GBps']:>12.1f} "
              f"{r['dense_GBps']:>11.1f}")


if __name__ == "__main__":
    main()
