"""Drafters for speculative decoding (runtime/engine.py: the verify step).

A drafter is ``callable(token_ids, k) -> list[int]``: given a request's tokens so far (prompt ids,
when the caller supplied them, followed by the generated ids) it proposes at most ``k`` tokens that
may come next.  The engine feeds the proposal through one batched verify step and keeps the prefix
the model agrees with, so a drafter can only change the speed, never the output.

A guided request (``LUMEN_SPEC_GUIDED``) has a drafter of its own that needs none of these: the
tokens its grammar forces (:meth:`lumen_amd.runtime.guided.Guide.forced`).  The engine asks the
drafter here only where the grammar forces nothing, and cuts its proposal at the first token the
grammar does not allow.
"""
from __future__ import annotations

import os
from typing import Callable, Optional, Sequence

import numpy as np

Drafter = Callable[[Sequence[int], int], list]

SPEC_TOKENS_DEFAULT = 3
SPEC_TOKENS_MAX = 7


class NgramDrafter:
    """Prompt-lookup drafting: the longest suffix (``max_n`` down to ``min_n`` tokens) of the
    history that also occurs earlier in it, the most recent occurrence if there are several; the
    proposal is what followed it there.  Needs no model; pays off where the output repeats its
    prompt or itself (transcriptions, structured captions, lists)."""

    def __init__(self, max_n: int = 4, min_n: int = 2):
        if not 1 <= min_n <= max_n:
            raise ValueError("NgramDrafter: 1 <= min_n <= max_n")
        self.max_n, self.min_n = int(max_n), int(min_n)

    def __call__(self, token_ids: Sequence[int], k: int) -> list:
        a = np.asarray(token_ids, dtype=np.int64)
        L = len(a)
        if k <= 0:
            return []
        for n in range(min(self.max_n, L - 1), self.min_n - 1, -1):
            # earlier occurrences start at s <= L - n - 1, so at least one token follows each
            hit = np.ones(L - n, dtype=bool)
            for j in range(n):
                hit &= a[j:L - n + j] == a[L - n + j]
            s = np.flatnonzero(hit)
            if len(s):
                e = int(s[-1]) + n
                return [int(t) for t in a[e:e + k]]
        return []


def spec_tokens_from_env(spec_tokens: Optional[int] = None) -> int:
    """draft tokens per verify step: the argument, else ``LUMEN_SPEC_TOKENS`` (default 3), in 1 .. 7"""
    n = int(os.environ.get("LUMEN_SPEC_TOKENS", SPEC_TOKENS_DEFAULT)) if spec_tokens is None else int(spec_tokens)
    return min(max(n, 1), SPEC_TOKENS_MAX)


def drafter_from_env() -> Optional[Drafter]:
    """``LUMEN_SPEC_DECODE=ngram``: the n-gram drafter; unset / ``0`` / ``off``: none"""
    name = os.environ.get("LUMEN_SPEC_DECODE", "").strip().lower()
    if name in ("", "0", "off", "none"):
        return None
    if name == "ngram":
        return NgramDrafter()
    raise ValueError(f"LUMEN_SPEC_DECODE={name!r}: expected 'ngram'")
