"""Per-workgroup timeline of the production ping-pong GEMM (tile 1629) on the ViT-L/14 b512 micro-batch
shapes (M = 256 * 257 rows), s_memrealtime (100 MHz): prologue (first K-tile landed), K-loop, epilogue, and
the gaps between a CU's consecutive tiles.  Epilogues: the LN-folded qkv / fc1 form (gemm_lnf, fc1 with
quick-GELU) and the bias + residual out-proj / fc2 form, as clip._block_steps issues them.

    python tools/gemm_pp_timeline.py [--tiles 1629,1829] [--tuning ID]
    python tools/gemm_pp_timeline.py --concurrent [--tiles 1839] [--tuning ID]

Several tile codes: each is timed and stamped in turn and its output compared with the first one's.
--tuning ID: every probe runs with the csrc/tuning.h switch ID at 0 and at 1, interleaved in this process.
--concurrent: the out-proj shape (bias + residual) and the fc1 shape (LN-fold + quick-GELU) run at the same
time on two streams, as the 2-stream tower runs them, so two different kernels' code is resident on
neighbouring CUs; both kernels' per-tile stamps are reported next to their stand-alone ones.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from lumen_amd import ops
from lumen_amd._native import hip_ops

SHAPES = [("qkv_lnf", 3072, 1024, "lnf"), ("out_res", 1024, 1024, "res"),
          ("fc1_lnf_gelu", 4096, 1024, "lnf_gelu"), ("fc2_res", 1024, 4096, "res")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", default="1629")
    ap.add_argument("--M", type=int, default=256 * 257)
    ap.add_argument("--tuning", type=int, default=None, help="csrc/tuning.h switch id: run both of its arms")
    ap.add_argument("--concurrent", action="store_true", help="out-proj and fc1 together on two streams")
    ap.add_argument("--reps", type=int, default=6, help="--concurrent: fc1 launches per stream window")
    ap.add_argument("--rounds", type=int, default=1, help="repeat the whole sweep (arms interleaved) this often")
    a = ap.parse_args()
    h = hip_ops()
    M = a.M
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(M, 1024, device=dev, generator=g).bfloat16()
    st = torch.stack([torch.full((M,), 0.9, device=dev), torch.full((M,), -0.01, device=dev)], 1).contiguous()
    arms = [None] if a.tuning is None else [0, 1]
    tiles = [int(t) for t in a.tiles.split(",")]
    base = h.set_tuning(a.tuning, 1) if a.tuning is not None else None
    problems = {}
    for name, N, K, kind in SHAPES:
        xa = x if K == 1024 else torch.randn(M, K, device=dev, generator=g).bfloat16()
        w = (torch.randn(N, K, device=dev, generator=g) * K ** -0.5).bfloat16()
        ca = torch.randn(2, N, device=dev, generator=g).contiguous()
        b = torch.randn(N, device=dev, generator=g).bfloat16()
        res = torch.randn(M, N, device=dev, generator=g).bfloat16() if not kind.startswith("lnf") else None
        problems[name] = (name, M, N, K, kind, xa, w, st, ca, b, res)
    try:
        first = {}
        for rnd in range(a.rounds):
            order = arms if rnd % 2 == 0 else arms[::-1]   # the later arm of a pair runs on the warmer chip
            for name, p in problems.items():
                for tile in tiles:
                    for arm in order:
                        if arm is not None:
                            h.set_tuning(a.tuning, arm)
                        first[name] = probe(h, *p, tile, first.get(name),
                                            "" if arm is None else f" tuning[{a.tuning}]={arm}")
            if a.concurrent:
                for tile in tiles:
                    for arm in order:
                        if arm is not None:
                            h.set_tuning(a.tuning, arm)
                        concurrent(h, problems["out_res"], problems["fc1_lnf_gelu"], tile, a.reps,
                                   "" if arm is None else f" tuning[{a.tuning}]={arm}")
    finally:
        if a.tuning is not None:
            h.set_tuning(a.tuning, base)


def runner(kind, xa, w, st, ca, b, res, tile, out):
    if kind.startswith("lnf"):
        act = "quick_gelu" if kind == "lnf_gelu" else None
        return lambda: ops.linear_lnf(xa, w, ca, st, act=act, tile=tile, out=out)
    return lambda: ops.linear(xa, w, b, residual=res, out=out, tile=tile)


def stamps(dbg, nt):
    d = dbg.view(nt, 4).cpu().double() * 10e-3   # us
    return d, (d[:, 1] - d[:, 0]), (d[:, 2] - d[:, 1]), (d[:, 3] - d[:, 2])


def probe(h, name, M, N, K, kind, xa, w, st, ca, b, res, tile, first, label):
        dev = "cuda"
        nt = ((M + 255) // 256) * ((N + 255) // 256)
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        dbg = torch.zeros(nt * 4, dtype=torch.int64, device=dev)
        run = runner(kind, xa, w, st, ca, b, res, tile, out)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(20):
            run()
        ev[1].record()
        torch.cuda.synchronize()
        ms = ev[0].elapsed_time(ev[1]) / 20
        h.gemm_set_dbg(dbg)
        run()
        torch.cuda.synchronize()
        h.gemm_set_dbg(dbg[:0])
        d, pro, loop, epi = stamps(dbg, nt)
        t0 = d[:, 0].min()
        span = (d[:, 3].max() - t0).item()
        # gap: sort tile ends; each later start pairs with the earliest unclaimed end (the CU it reuses)
        ends = (d[:, 3] - t0).sort().values
        starts = (d[:, 0] - t0).sort().values
        gaps = (starts[256:] - ends[:nt - 256]) if nt > 256 else torch.zeros(1)
        tiles_per_cu = nt / 256
        busy = (d[:, 3] - d[:, 0]).sum().item() / 256
        tf = 2 * M * N * K / (ms * 1e-3) / 1e12
        diff = 0.0 if first is None else ((out.float() - first.float()).abs().max() /
                                          first.float().abs().max()).item()
        print(f"{name:14s} tile {tile}{label} diff {diff:.2e} M={M} N={N} K={K} tiles={nt} ({tiles_per_cu:.2f}/CU): {ms * 1e3:.1f} us ({tf:.0f} TF); "
              f"per tile median prologue {pro.median():.2f} / K-loop {loop.median():.2f} / epilogue {epi.median():.2f} us "
              f"(p90 {pro.quantile(.9):.2f} / {loop.quantile(.9):.2f} / {epi.quantile(.9):.2f}); "
              f"dispatch gap median {gaps.median():.2f} us; span {span:.1f} us, CU-busy {busy:.1f} us", flush=True)
        return out.clone() if first is None else first


def concurrent(h, pa, pb, tile, reps, label):
    """pa (out-proj) on one stream, pb (fc1) on another, each stream a back-to-back run of its GEMM sized to
    the same FLOPs (N_b / N_a launches of pa per launch of pb), every launch stamped into a buffer of its
    own.  Reported per kernel: the stamps over the middle half of its launches, and how many tiles of the
    OTHER kernel were in flight at the middle of each of those tiles (of 256 CUs, one workgroup per CU).
    Two streams that share a hardware queue run their windows one after the other (0 tiles in flight): the
    window is then taken again with the next stream as the second one."""
    dev = "cuda"
    info = []
    counts = [reps * max(1, pb[2] * pb[3] // (pa[2] * pa[3])), reps]
    for (name, M, N, K, kind, xa, w, st, ca, b, res), n in zip((pa, pb), counts):
        nt = ((M + 255) // 256) * ((N + 255) // 256)
        out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        dbg = torch.zeros(n, nt * 4, dtype=torch.int64, device=dev)
        info.append([name, nt, 2 * M * N * K, dbg, runner(kind, xa, w, st, ca, b, res, tile, out), None])
    for _, _, _, _, run, _ in info:
        run()
    torch.cuda.synchronize()
    if not _STREAMS:
        _STREAMS.extend(torch.cuda.Stream() for _ in range(4))
    for second in (1, 2, 3):
        info[0][5], info[1][5] = _STREAMS[0], _STREAMS[second]
        if _window(h, info, counts, tile, label) > 0:
            break


_STREAMS = []


def _window(h, info, counts, tile, label):
    for _ in range(2):                                               # the first window warms up; the second is read
        evs = []
        for (name, nt, fl, dbg, run, s), n in zip(info, counts):      # enqueue only: both streams then drain together
            with torch.cuda.stream(s):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(n):
                    h.gemm_set_dbg(dbg[i])
                    run()
                e1.record()
            evs.append((e0, e1))
        h.gemm_set_dbg(info[0][3][0, :0])
        torch.cuda.synchronize()
    ds = [dbg.view(n, nt, 4).cpu().double() * 10e-3 for (_, nt, _, dbg, _, _), n in zip(info, counts)]   # us
    overlap = 0.0
    for i, ((name, nt, fl, dbg, run, s), n) in enumerate(zip(info, counts)):
        d = ds[i][n // 4:n - n // 4].reshape(-1, 4)
        o = ds[1 - i].reshape(-1, 4)
        pro, loop, epi = d[:, 1] - d[:, 0], d[:, 2] - d[:, 1], d[:, 3] - d[:, 2]
        mid = ((d[:, 0] + d[:, 3]) / 2).contiguous()
        other = (torch.searchsorted(o[:, 0].sort().values, mid) - torch.searchsorted(o[:, 3].sort().values, mid)).double()
        overlap = max(overlap, other.median().item())
        us = evs[i][0].elapsed_time(evs[i][1]) * 1e3 / n
        print(f"concurrent {name:14s} tile {tile}{label} {n} launches beside {info[1 - i][0]}: {us:.1f} us per GEMM in its stream "
              f"({fl / (us * 1e-6) / 1e12:.0f} TF); per tile median prologue {pro.median():.2f} / K-loop {loop.median():.2f} / "
              f"epilogue {epi.median():.2f} us (p90 {pro.quantile(.9):.2f} / {loop.quantile(.9):.2f} / {epi.quantile(.9):.2f}); "
              f"tiles of the other kernel in flight beside a tile: median {other.median():.0f}, p10 {other.quantile(.1):.0f}",
              flush=True)
    return overlap


if __name__ == "__main__":
    main()
