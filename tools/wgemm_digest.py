"""Bit digests of the weight-only GEMMs (bf16 skinny, fp8, 4-bit) over every kernel instantiation
their dispatchers can select.

A fixed, seeded list of small cases runs through ops.linear / ops.linear_dec on the GPU; one
sha256 of the output bytes is printed per case (and of the ssq tensor for ssq_out cases).  Two
builds that launch the same kernels with the same summation orders print the same lines, so a
refactor of csrc/gemm_skinny.hip, gemm_w8.hip, gemm_w4.hip or their shared headers is checked
with a plain diff of two runs.

    python tools/wgemm_digest.py [OUT.txt]
"""
import hashlib
import os
import sys
import zlib

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lumen_amd import ops  # noqa: E402
from lumen_amd._native import load_hip  # noqa: E402

DEV = "cuda"   # formats below: "bf16", "fp8", "w4g32" / "w4g128" (4-bit, group 32 / 128)

# Decode kernels: (formats, M, N, K list).  N picks the column tiles per wave (64 | N: 4, 32 | N: 2,
# else 1); K picks the split (none below 2 x the minimum K per split) and the tails.
ROWS_K8 = (896, 1088, 4864, 7168)        # fp8 1024-wide steps: short row, step + tail, chunks + tail, steady state
ROWS_K4 = (896, 2176, 4864, 14336)       # 4-bit 2048-wide steps
DECODE = [
    # row-streaming GEMVs <1, .> <2, .> <4, 1>
    (("fp8",), 1, 48, ROWS_K8), (("fp8",), 2, 64, ROWS_K8), (("fp8",), 3, 80, ROWS_K8),
    (("w4g32", "w4g128"), 1, 48, ROWS_K4), (("w4g32", "w4g128"), 2, 64, ROWS_K4),
    (("w4g32", "w4g128"), 4, 80, ROWS_K4),
    # fp8 MFMA GEMV, tpw 4 / 2 / 1: unsplit, split, preloaded (K <= 4096) and fallback rstd
    (("fp8",), 5, 192, (448, 896, 4096, 4864)), (("fp8",), 16, 96, (448, 896, 4096, 4864)),
    (("fp8",), 9, 48, (448, 896, 4096, 4864)),
    # 16-column skinny kernel: bf16 MT 1 / 2, fp8 MT 2; unsplit and split
    (("bf16",), 5, 48, (896, 4864)), (("bf16", "fp8"), 17, 48, (896, 4864)), (("bf16", "fp8"), 32, 64, (896, 4864)),
    # 4-bit skinny MT 1 x tpw 4 / 2 / 1, MT 2 x tpw 2 / 1: unsplit, split
    (("w4g32", "w4g128"), 5, 192, (384, 4096, 4864)), (("w4g32", "w4g128"), 16, 96, (384, 4096, 4864)),
    (("w4g32", "w4g128"), 9, 48, (384, 4096, 4864)), (("w4g32", "w4g128"), 17, 96, (384, 4096, 4864)),
    (("w4g32", "w4g128"), 32, 48, (384, 4096, 4864)),
    # ... and a partial 128-wide block (G = 32 only), unsplit and in the last split
    (("w4g32",), 7, 64, (928, 4896)), (("w4g32",), 20, 48, (928, 4896)),
]
# Prefill tiles: 64x64 (ragged M, smallest M) and 128x128 (>= 256 tiles, ragged M); the 4-bit
# G = 32 cases end in a half k tile
PREFILL = [
    (("fp8", "w4g128"), 200, 192, (1024,)), (("w4g32",), 200, 192, (928,)), (("fp8", "w4g32", "w4g128"), 33, 96, (896,)),
    (("fp8", "w4g128"), 2000, 2048, (128,)), (("w4g32",), 2000, 2048, (160,)),
]
EPI_DECODE = ("f32", "bias_res", "bias32", "glu", "glu_norm", "norm_ssq", "res_ssq")
EPI_PREFILL = ("f32", "bias_res", "glu")


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


_weights = {}


def weight(fmt, N, K):
    if (fmt, N, K) not in _weights:
        w = torch.randn(N, K, generator=_gen("w", N, K)) * K ** -0.5
        if fmt == "bf16":
            q, s = w.bfloat16(), None
        elif fmt == "fp8":
            q, s = ops.quantize_fp8_rows(w)
        else:
            q, s = ops.quantize_w4_rows(w, int(fmt[3:]))
        _weights[(fmt, N, K)] = (q.to(DEV), s.to(DEV) if s is not None else None)
    return _weights[(fmt, N, K)]


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def run(fmt, M, N, K, epi):
    w, s = weight(fmt, N, K)
    g = _gen("x", M, N, K)
    x = torch.randn(M, K, generator=g).bfloat16().to(DEV)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g).bfloat16().to(DEV)
    if epi == "f32":
        return [ops.linear(x, w, w_scale=s, out_dtype=torch.float32)]
    if epi == "bias_res":
        return [ops.linear(x, w, bias.bfloat16().to(DEV), residual=res, w_scale=s)]
    if epi == "bias32":
        return [ops.linear(x, w, bias.to(DEV), w_scale=s, out_dtype=torch.float32)]
    if epi == "glu":
        return [ops.linear(x, w, glu=True, w_scale=s)]
    if epi == "glu_norm":       # rstd from the rows of x
        return [ops.linear_dec(x, w, s, glu=True, norm_eps=1e-5)]
    if epi == "norm_ssq":       # rstd from the producer's per-tile sums of squares
        ssq = (x.float() ** 2).view(M, K // 16, 16).sum(-1).contiguous()
        return [ops.linear_dec(x, w, s, norm_eps=1e-5, ssq_in=ssq)]
    ssq_out = torch.zeros(M, N // 16, device=DEV)
    return [ops.linear_dec(x, w, s, residual=res, ssq_out=ssq_out), ssq_out]


def cases():
    for group, epis in ((DECODE, EPI_DECODE), (PREFILL, EPI_PREFILL)):
        for fmts, M, N, Ks in group:
            for fmt in fmts:
                for K in Ks:
                    for epi in epis:
                        if epi == "norm_ssq" and K % 64:
                            continue          # the kernels read the sums of squares four tiles at a time
                        yield fmt, M, N, K, epi


def main():
    load_hip(required=True)
    torch.manual_seed(0)
    lines = []
    for fmt, M, N, K, epi in cases():
        outs = run(fmt, M, N, K, epi)
        torch.cuda.synchronize()
        lines.append(f"{fmt} M{M} N{N} K{K} {epi} " + " ".join(sha(o) for o in outs))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
