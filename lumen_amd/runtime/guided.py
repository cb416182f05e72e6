"""Guided decoding: regular expressions, choices and a JSON-schema subset compiled to a byte DFA
and to per-state bitmaps of the tokens that may follow.

The device sampler (csrc/sampler.hip, guided form) draws among the tokens whose bit is set in the
row of the request's grammar state and then walks the drawn token's bytes through the DFA, so a
look-ahead step constrains token n + 1 before the host has read token n.  The host keeps the same
state (:meth:`Guide.walk`) for the steps it feeds and for the host sampling path.

Pipeline: pattern -> AST over code points -> Thompson NFA over UTF-8 bytes -> subset construction
-> Moore minimisation -> states that cannot reach an accepting state are deleted (a live state
always has a way to finish).  ``choice`` and ``json_schema`` lower to a regex first.

Regex syntax (anchored, full match): literals, ``.`` (any code point but ``\\n``), classes and
negated classes with ranges, ``\\d \\w \\s`` and their negations (ASCII sense), ``\\n \\t \\r \\f \\v``,
``\\xHH``, ``\\uHHHH``, escaped punctuation, groups ``( )`` and ``(?: )``, ``|``, ``* + ?``, ``{m}``,
``{m,}``, ``{m,n}``.  ``.`` and negated classes match whole well-formed UTF-8 sequences.  Anything
else -- back-references, look-around, lazy or possessive quantifiers, anchors, flags, named
groups -- raises :class:`GuideError` with the offset.

JSON-schema subset: ``object`` with ``properties`` in the listed order (those named in ``required``,
or all without it; no additional properties), ``string`` (``minLength``, ``maxLength``, ``enum``,
``pattern``), ``integer``, ``number``, ``boolean``, ``null``, ``enum`` / ``const`` of scalars, ``array`` with
``items``, ``minItems``, ``maxItems``, ``anyOf``, a list of types, nesting.  Whitespace: one optional
space after ``:`` and after ``,`` and nothing else.  Other keywords raise :class:`GuideError` naming
the keyword; the annotations ``title``, ``description``, ``default``, ``examples``, ``$schema`` and ``$id``
are ignored.

A grammar may have at most ``LUMEN_GUIDED_MAX_STATES`` states after minimisation (default 2048;
the four-property photo-tag schema of tools/guided_bench.py needs a few hundred).

A request cut by ``max_new_tokens`` ends with reason ``length`` and its text may be an incomplete
match (always a prefix of one).  EOS ids are expected to be special tokens.
"""
from __future__ import annotations

import json
import os
import threading
from collections import OrderedDict
from typing import Optional, Sequence

import numpy as np

MAX_CP = 0x10FFFF
_NFA_CAP = 400_000          # Thompson states: bounded repetitions are unrolled


class GuideError(ValueError):
    """the grammar is outside the supported subset, too large, or the tokenizer is unsupported"""


def max_states() -> int:
    return int(os.environ.get("LUMEN_GUIDED_MAX_STATES", 2048))


# ------------------------------------------------------------------ code-point sets
def _norm(rs):
    """sorted disjoint code-point ranges without the surrogates (not encodable as UTF-8)"""
    out = []
    for lo, hi in sorted(rs):
        for a, b in ((lo, min(hi, 0xD7FF)), (max(lo, 0xE000), hi)):
            if a > b:
                continue
            if out and a <= out[-1][1] + 1:
                out[-1] = (out[-1][0], max(out[-1][1], b))
            else:
                out.append((a, b))
    return out


def _neg(rs):
    out, at = [], 0
    for lo, hi in _norm(rs):
        if lo > at:
            out.append((at, lo - 1))
        at = hi + 1
    if at <= MAX_CP:
        out.append((at, MAX_CP))
    return _norm(out)


_DIGIT = [(48, 57)]
_WORD = [(48, 57), (65, 90), (95, 95), (97, 122)]
_SPACE = [(9, 13), (32, 32)]
_CLASS_ESC = {"d": _DIGIT, "w": _WORD, "s": _SPACE}
_CHAR_ESC = {"n": 10, "t": 9, "r": 13, "f": 12, "v": 11, "0": 0}


# ------------------------------------------------------------------ parser
class _Parser:
    """AST: ("set", ranges) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, m, n or None)"""

    def __init__(self, pat: str):
        self.p, self.i = pat, 0

    def err(self, msg: str, at: Optional[int] = None):
        raise GuideError(f"regex: {msg} at offset {self.i if at is None else at}")

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.err("unbalanced ')'")
        return node

    def alt(self):
        parts = [self.cat()]
        while self.i < len(self.p) and self.p[self.i] == "|":
            self.i += 1
            parts.append(self.cat())
        return parts[0] if len(parts) == 1 else ("alt", parts)

    def cat(self):
        items = []
        while self.i < len(self.p) and self.p[self.i] not in "|)":
            items.append(self.quantified())
        return ("cat", items)

    def quantified(self):
        at = self.i
        node = self.atom()
        while self.i < len(self.p):
            c = self.p[self.i]
            if c == "*":
                m, n = 0, None
            elif c == "+":
                m, n = 1, None
            elif c == "?":
                m, n = 0, 1
            elif c == "{":
                q = self.braces()
                if q is None:
                    break
                m, n = q
            else:
                break
            if c != "{":
                self.i += 1
            if self.i < len(self.p) and self.p[self.i] in "?+":
                self.err("lazy and possessive quantifiers are not supported")
            if n is not None and n < m:
                self.err("bad repetition bounds", at)
            node = ("rep", node, m, n)
        return node

    def braces(self):
        """{m} {m,} {m,n} at self.i -> (m, n) and the position moves past it; anything else: None
        (the brace is a literal, as in Python's re)"""
        j = self.p.find("}", self.i)
        if j < 0:
            return None
        body = self.p[self.i + 1:j]
        a, comma, b = body.partition(",")
        if not a.isdigit() or (b and not b.isdigit()) or not a.isascii() or not b.isascii():
            return None
        self.i = j + 1
        m = int(a)
        return (m, m) if not comma else (m, int(b) if b else None)

    def atom(self):
        c = self.p[self.i]
        if c == "(":
            at = self.i
            self.i += 1
            if self.p.startswith("?:", self.i):
                self.i += 2
            elif self.i < len(self.p) and self.p[self.i] == "?":
                self.err("look-around, flags and named groups are not supported", at)
            node = self.alt()
            if self.i >= len(self.p) or self.p[self.i] != ")":
                self.err("missing ')'", at)
            self.i += 1
            return node
        if c == "[":
            return self.cls()
        if c == ".":
            self.i += 1
            return ("set", _neg([(10, 10)]))
        if c in "^$":
            self.err("anchors are not supported (the match is anchored and full)")
        if c in "*+?":
            self.err("nothing to repeat")
        if c == "\\":
            r = self.escape(False)
            return ("set", _norm(r))
        self.i += 1
        return ("set", [(ord(c), ord(c))])

    def escape(self, in_class: bool):
        """the escape at self.i -> code-point ranges"""
        at = self.i
        self.i += 1
        if self.i >= len(self.p):
            self.err("trailing backslash", at)
        c = self.p[self.i]
        self.i += 1
        if c in _CLASS_ESC:
            return list(_CLASS_ESC[c])
        if c in "DWS":
            return _neg(_CLASS_ESC[c.lower()])
        if c in "xu":
            n = 2 if c == "x" else 4
            h = self.p[self.i:self.i + n]
            if len(h) != n or any(ch not in "0123456789abcdefABCDEF" for ch in h):
                self.err("bad hexadecimal escape", at)
            self.i += n
            return [(int(h, 16),) * 2]
        if c in _CHAR_ESC and not (c == "0" and self.p[self.i:self.i + 1].isdigit()):
            return [(_CHAR_ESC[c],) * 2]
        if c.isdigit():
            self.err("back-references are not supported", at)
        if c == "b" and in_class:
            return [(8, 8)]
        if c in "bBAZzGkpPNU" or c.isalnum():
            self.err(f"escape \\{c} is not supported", at)
        return [(ord(c), ord(c))]

    def cls(self):
        at = self.i
        self.i += 1
        neg = self.p.startswith("^", self.i)
        self.i += neg
        rs, first = [], True
        while True:
            if self.i >= len(self.p):
                self.err("missing ']'", at)
            c = self.p[self.i]
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            if c == "\\":
                lo = self.escape(True)
            else:
                self.i += 1
                lo = [(ord(c), ord(c))]
            single = len(lo) == 1 and lo[0][0] == lo[0][1]
            if single and self.p.startswith("-", self.i) and self.i + 1 < len(self.p) and self.p[self.i + 1] != "]":
                self.i += 1
                if self.p[self.i] == "\\":
                    hi = self.escape(True)
                else:
                    hi = [(ord(self.p[self.i]),) * 2]
                    self.i += 1
                if not (len(hi) == 1 and hi[0][0] == hi[0][1]) or hi[0][0] < lo[0][0]:
                    self.err("bad character range", at)
                rs.append((lo[0][0], hi[0][0]))
            else:
                rs.extend(lo)
        rs = _neg(rs) if neg else _norm(rs)
        if not rs:
            self.err("empty character class", at)
        return ("set", rs)


# ------------------------------------------------------------------ UTF-8 byte sequences of a range
def _enc(cp: int) -> bytes:
    return chr(cp).encode("utf-8")


def _utf8_seqs(lo: int, hi: int):
    """sequences of byte ranges that match exactly the UTF-8 encodings of lo .. hi (no surrogates)"""
    for cut in (0x7F, 0x7FF, 0xFFFF):
        if lo <= cut < hi:
            yield from _utf8_seqs(lo, cut)
            yield from _utf8_seqs(cut + 1, hi)
            return
    if hi <= 0x7F:
        yield [(lo, hi)]
        return
    n = len(_enc(lo))
    for i in range(1, n):
        m = (1 << (6 * i)) - 1
        if lo & ~m != hi & ~m:
            if lo & m != 0:
                yield from _utf8_seqs(lo, lo | m)
                yield from _utf8_seqs((lo | m) + 1, hi)
                return
            if hi & m != m:
                yield from _utf8_seqs(lo, (hi & ~m) - 1)
                yield from _utf8_seqs(hi & ~m, hi)
                return
    yield list(zip(_enc(lo), _enc(hi)))


# ------------------------------------------------------------------ NFA
class _NFA:
    def __init__(self):
        self.eps: list = []
        self.tr: list = []       # per state: [(byte lo, byte hi, target)]

    def new(self) -> int:
        if len(self.eps) >= _NFA_CAP:
            raise GuideError("regex: the grammar is too large (bounded repetitions are unrolled)")
        self.eps.append([])
        self.tr.append([])
        return len(self.eps) - 1

    def build(self, node) -> tuple:
        """-> (entry, exit) of a fragment"""
        kind = node[0]
        if kind == "set":
            a, b = self.new(), self.new()
            for lo, hi in node[1]:
                for seq in _utf8_seqs(lo, hi):
                    s = a
                    for k, (x, y) in enumerate(seq):
                        t = b if k == len(seq) - 1 else self.new()
                        self.tr[s].append((x, y, t))
                        s = t
            return a, b
        if kind == "cat":
            a = self.new()
            s = a
            for sub in node[1]:
                x, y = self.build(sub)
                self.eps[s].append(x)
                s = y
            return a, s
        if kind == "alt":
            a, b = self.new(), self.new()
            for sub in node[1]:
                x, y = self.build(sub)
                self.eps[a].append(x)
                self.eps[y].append(b)
            return a, b
        _, sub, m, n = node
        a = self.new()
        s = a
        for _ in range(m):
            x, y = self.build(sub)
            self.eps[s].append(x)
            s = y
        if n is None:
            x, y = self.build(sub)
            h = self.new()
            self.eps[s].append(h)
            self.eps[h].append(x)
            self.eps[y].append(h)
            return a, h
        end = self.new()
        for _ in range(n - m):
            x, y = self.build(sub)
            self.eps[s].append(x)
            self.eps[s].append(end)
            s = y
        self.eps[s].append(end)
        return a, end


def _closure(nfa: _NFA, states) -> frozenset:
    seen, stack = set(states), list(states)
    while stack:
        for t in nfa.eps[stack.pop()]:
            if t not in seen:
                seen.add(t)
                stack.append(t)
    return frozenset(seen)


def _subset(nfa: _NFA, start: int, final: int, cap: int):
    """-> (dfa int32 [S, 256] with -1 = dead, accept bool [S]); state 0 is the start"""
    s0 = _closure(nfa, [start])
    index, rows, order = {s0: 0}, [], [s0]
    k = 0
    while k < len(order):
        cur = order[k]
        k += 1
        row = np.full(256, -1, np.int32)
        trs = [t for s in cur for t in nfa.tr[s]]
        if trs:
            cuts = sorted({t[0] for t in trs} | {t[1] + 1 for t in trs})
            for lo, nxt in zip(cuts, cuts[1:]):
                tgt = {t[2] for t in trs if t[0] <= lo <= t[1]}
                if not tgt:
                    continue
                key = _closure(nfa, tgt)
                j = index.get(key)
                if j is None:
                    j = index[key] = len(order)
                    order.append(key)
                    if j >= cap:
                        raise GuideError(f"the grammar needs more than {cap} states before minimisation "
                                         f"(LUMEN_GUIDED_MAX_STATES = {max_states()})")
                row[lo:nxt] = j
        rows.append(row)
    return np.stack(rows), np.array([final in s for s in order], bool)


def _minimise(dfa: np.ndarray, accept: np.ndarray):
    """trim (forward from the start is given; backward from the accepting states) and merge
    equivalent states (Moore's refinement over byte classes).  -> (dfa, accept), start = 0"""
    S = dfa.shape[0]
    # states that can reach an accepting state
    live = accept.copy()
    ext = np.concatenate([live, [False]])
    while True:
        ext[:S] = live
        new = live | ext[dfa].any(1)           # dfa = -1 indexes the False at the end
        if (new == live).all():
            break
        live = new
    if not live[0]:
        raise GuideError("the grammar matches nothing")
    dfa = np.where(np.concatenate([live, [False]])[dfa], dfa, -1)
    # forward reachability over live states
    reach = np.zeros(S, bool)
    reach[0] = True
    front = np.array([0])
    while len(front):
        nxt = np.unique(dfa[front])
        nxt = nxt[nxt >= 0]
        front = nxt[~reach[nxt]]
        reach[front] = True
    keep = np.nonzero(reach & live)[0]
    ren = np.full(S + 1, -1, np.int64)
    ren[keep] = np.arange(len(keep))
    dfa, accept = ren[dfa[keep]], accept[keep]
    S = len(keep)
    # byte classes: identical columns
    cols, inv = np.unique(dfa.T, axis=0, return_inverse=True)
    red = np.ascontiguousarray(cols.T)         # [S, classes]
    cls = accept.astype(np.int64)
    ncls = len(np.unique(cls))
    while True:
        ext = np.concatenate([cls, [-1]])
        sig = np.ascontiguousarray(np.concatenate([cls[:, None], ext[red]], 1))
        _, first, new = np.unique(sig.view(np.dtype((np.void, sig.dtype.itemsize * sig.shape[1]))).ravel(),
                                  return_index=True, return_inverse=True)
        n = len(first)
        cls = new.ravel()
        if n == ncls:
            break
        ncls = n
    # renumber so that the start's class is 0 and the order is that of first appearance
    _, first = np.unique(cls, return_index=True)
    order = np.argsort(first)                  # classes by first member
    rank = np.empty(ncls, np.int64)
    rank[order] = np.arange(ncls)
    cls = rank[cls]
    rep = np.sort(first)
    ext = np.concatenate([cls, [-1]])
    out = ext[red[rep]][:, inv.ravel()]
    return out.astype(np.int32), accept[rep]


def compile_regex(pattern: str, cap: Optional[int] = None):
    """-> (dfa int16 [S, 256] with -1 = dead, accept bool [S]); state 0 is the start state.  Every
    state can reach an accepting one."""
    cap = max_states() if cap is None else cap
    if not isinstance(pattern, str):
        raise GuideError("regex: the pattern must be a string")
    ast = _Parser(pattern).parse()
    nfa = _NFA()
    a, b = nfa.build(ast)
    dfa, accept = _subset(nfa, a, b, max(8 * cap, 4096))
    dfa, accept = _minimise(dfa, accept)
    if dfa.shape[0] > cap:
        raise GuideError(f"the grammar needs {dfa.shape[0]} states, LUMEN_GUIDED_MAX_STATES allows {cap}")
    return dfa.astype(np.int16), accept


# ------------------------------------------------------------------ front ends
def regex_escape(s: str) -> str:
    return "".join("\\" + c if c in "\\.[](){}|*+?^$-/" else
                   "\\n" if c == "\n" else "\\r" if c == "\r" else "\\t" if c == "\t" else c for c in s)


def choice_regex(choices: Sequence[str]) -> str:
    if not isinstance(choices, (list, tuple)) or not choices or not all(isinstance(c, str) and c for c in choices):
        raise GuideError("choice: a non-empty list of non-empty strings")
    return "(" + "|".join(regex_escape(c) for c in choices) + ")"


_STR_CHAR = r'([^"\\\x00-\x1f]|\\(["\\/bfnrt]|u[0-9a-fA-F]{4}))'
_INT = r"-?(0|[1-9][0-9]*)"
_NUM = _INT + r"(\.[0-9]+)?([eE][+\-]?[0-9]+)?"
_IGNORED = {"title", "description", "default", "examples", "$schema", "$id", "$comment"}
_KEYS = {"object": {"properties", "required", "additionalProperties"},
         "string": {"minLength", "maxLength", "enum", "pattern"},
         "array": {"items", "minItems", "maxItems"},
         "integer": set(), "number": set(), "boolean": set(), "null": set()}


def _scalar(v) -> str:
    if v is None or isinstance(v, (bool, int, float, str)):
        return regex_escape(json.dumps(v, ensure_ascii=False))
    raise GuideError("json_schema: enum / const hold scalars only")


def schema_regex(schema) -> str:
    """the JSON-schema subset (see the module text) as a regex"""
    if schema is True or schema == {}:
        raise GuideError("json_schema: an unconstrained value ({} or true) is not supported; give a type")
    if not isinstance(schema, dict):
        raise GuideError("json_schema: a schema is an object")
    keys = set(schema) - _IGNORED
    if "const" in keys:
        return _scalar(schema["const"])
    if "anyOf" in keys:
        if keys - {"anyOf"}:
            raise GuideError(f"json_schema: keyword {sorted(keys - {'anyOf'})[0]!r} next to anyOf is not supported")
        subs = schema["anyOf"]
        if not isinstance(subs, list) or not subs:
            raise GuideError("json_schema: anyOf holds a non-empty list")
        return "(" + "|".join(schema_regex(s) for s in subs) + ")"
    ty = schema.get("type")
    if isinstance(ty, list):          # a list of types: each type with the keywords that belong to it
        known = set().union(*(_KEYS.get(t, set()) for t in ty)) | {"enum"}
        if keys - {"type"} - known:
            raise GuideError(f"json_schema: keyword {sorted(keys - {'type'} - known)[0]!r} is not supported")
        return "(" + "|".join(schema_regex({**{k: v for k, v in schema.items() if k in _KEYS.get(t, ())}, "type": t})
                              for t in ty) + ")"
    if ty is None and "enum" in keys:
        if keys - {"enum"}:
            raise GuideError(f"json_schema: keyword {sorted(keys - {'enum'})[0]!r} is not supported")
        return "(" + "|".join(_scalar(v) for v in schema["enum"]) + ")"
    if ty not in _KEYS:
        bad = sorted(keys - {"type"})
        raise GuideError(f"json_schema: keyword {bad[0]!r} is not supported" if ty is None and bad
                         else f"json_schema: type {ty!r} is not supported")
    extra = keys - {"type"} - _KEYS[ty] - ({"enum"} if ty != "object" and ty != "array" else set())
    if extra:
        raise GuideError(f"json_schema: keyword {sorted(extra)[0]!r} is not supported for type {ty!r}")
    if "enum" in keys:
        return "(" + "|".join(_scalar(v) for v in schema["enum"]) + ")"
    if ty == "string":
        if "pattern" in keys:
            if keys & {"minLength", "maxLength"}:
                raise GuideError("json_schema: keyword 'pattern' together with a length bound is not supported")
            return '"(' + schema["pattern"] + ')"'
        lo, hi = int(schema.get("minLength", 0)), schema.get("maxLength")
        q = "*" if lo == 0 and hi is None else "{%d,%s}" % (lo, "" if hi is None else int(hi))
        return '"' + _STR_CHAR + q + '"'
    if ty == "integer":
        return _INT
    if ty == "number":
        return _NUM
    if ty == "boolean":
        return "(true|false)"
    if ty == "null":
        return "null"
    if ty == "array":
        if "items" not in schema:
            raise GuideError("json_schema: an array needs 'items'")
        item = schema_regex(schema["items"])
        lo, hi = int(schema.get("minItems", 0)), schema.get("maxItems")
        if hi is not None and int(hi) < max(lo, 0):
            raise GuideError("json_schema: maxItems below minItems")
        if hi is not None and int(hi) == 0:
            return r"\[\]"
        more = "(, ?%s){%d,%s}" % (item, max(lo - 1, 0), "" if hi is None else int(hi) - 1)
        body = "(" + item + ")" + more
        return r"\[(" + body + (")?" if lo == 0 else ")") + r"\]"
    props = schema.get("properties", {})
    if schema.get("additionalProperties", False) is not False:
        raise GuideError("json_schema: keyword 'additionalProperties' other than false is not supported")
    if not isinstance(props, dict):
        raise GuideError("json_schema: properties is an object")
    req = schema.get("required")
    if req is not None and [k for k in req if k not in props]:
        raise GuideError("json_schema: a required property is missing from properties")
    names = [k for k in props if req is None or k in req]
    parts = [regex_escape(json.dumps(k, ensure_ascii=False)) + ": ?(" + schema_regex(props[k]) + ")" for k in names]
    return r"\{" + ", ?".join(parts) + r"\}"


def lower(kind: str, spec) -> str:
    """the regex of a guide: ``kind`` is "regex" (a pattern), "choice" (a list of strings, or its
    JSON text) or "json_schema" (a schema, or its JSON text)"""
    if kind == "regex":
        return spec
    if kind in ("choice", "json_schema") and isinstance(spec, str):
        try:
            spec = json.loads(spec)
        except ValueError as e:
            raise GuideError(f"{kind}: malformed JSON ({e})") from None
    if kind == "choice":
        return choice_regex(spec)
    if kind == "json_schema":
        return schema_regex(spec)
    raise GuideError(f"unknown guide kind {kind!r}: regex, choice or json_schema")


def check(kind: str, spec) -> str:
    """lower and parse without compiling: raises GuideError for what is outside the supported syntax
    (not for the state cap); returns the regex"""
    text = lower(kind, spec)
    if not isinstance(text, str):
        raise GuideError("regex: the pattern must be a string")
    _Parser(text).parse()
    return text


# ------------------------------------------------------------------ token tables
_BYTES_INDEX: dict = {}      # id(token_bytes) -> (token_bytes, {bytes: lowest id}, longest token)


def _bytes_index(token_bytes: Sequence[bytes]):
    """({bytes: the lowest id with these bytes}, length of the longest token) of a vocabulary, built
    once per vocabulary object (the guides of an engine share one)"""
    hit = _BYTES_INDEX.get(id(token_bytes))
    if hit is None or hit[0] is not token_bytes:
        index: dict = {}
        for t, b in enumerate(token_bytes):
            if b:
                index.setdefault(bytes(b), t)
        if len(_BYTES_INDEX) >= 8:
            _BYTES_INDEX.clear()
        hit = _BYTES_INDEX[id(token_bytes)] = (token_bytes, index, max(map(len, index), default=0))
    return hit[1], hit[2]


class Guide:
    """A compiled grammar over one vocabulary.

    ``dfa`` int16 [S, 256] (-1 = dead), ``accept`` bool [S], ``allow`` int32 [S, ceil(V / 32)]: bit t
    of row s is set exactly when walking token t's bytes from s stays alive (a token without bytes
    is never allowed); the ids in ``eos_ids`` are allowed exactly in the accepting states; bits at
    and beyond V are zero.  ``start`` is the start state."""

    def __init__(self, kind, text, dfa, accept, allow, token_bytes, eos_ids):
        self.kind, self.text = kind, text
        self.dfa, self.accept, self.allow = dfa, accept, allow
        self.start = 0
        self.token_bytes = token_bytes
        self.eos_ids = frozenset(int(t) for t in eos_ids)
        self.V = len(token_bytes)
        self._forced: dict = {}      # state -> the tokens of its forced byte run (:meth:`forced`)

    @property
    def n_states(self) -> int:
        return self.dfa.shape[0]

    def walk(self, state: int, token: int) -> int:
        """the state after ``token``; EOS or a token without bytes leaves it; -1: the token is not
        allowed here"""
        if state < 0 or token in self.eos_ids or not 0 <= token < self.V:
            return state
        for b in self.token_bytes[token]:
            state = int(self.dfa[state, b])
            if state < 0:
                return -1
        return state

    def allows(self, state: int, token: int) -> bool:
        return 0 <= token < self.V and bool((int(self.allow[state, token >> 5]) >> (token & 31)) & 1)

    def forced(self, state: int, k: int) -> tuple:
        """At most ``k`` tokens that spell the bytes the grammar forces from ``state``: the DFA is
        followed while the state is not accepting (there EOS is an alternative) and exactly one byte
        has a live transition, and that byte run is cut into tokens greedily -- at each point the
        longest token whose bytes are a prefix of the rest of the run and that the state allows, the
        lowest id among tokens with equal bytes -- until no whole token fits.  Never EOS, never a
        token without bytes.  Deterministic and cached per state: the draft of speculative decoding
        for a guided request (the only way the model can reject it is another tokenisation of the
        same bytes)."""
        if k <= 0 or not 0 <= state < self.n_states:
            return ()
        hit = self._forced.get(state)
        if hit is None:
            run, s = [], state
            while not self.accept[s] and len(run) < self.n_states:
                live = np.flatnonzero(self.dfa[s] >= 0)
                if len(live) != 1:
                    break
                run.append(int(live[0]))
                s = int(self.dfa[s, live[0]])
            index, longest = _bytes_index(self.token_bytes)
            run, out, at, s = bytes(run), [], 0, state
            while at < len(run):
                for n in range(min(longest, len(run) - at), 0, -1):
                    t = index.get(run[at:at + n])
                    if t is not None and t not in self.eos_ids and self.allows(s, t):
                        break
                else:
                    break
                out.append(t)
                at += n
                s = self.walk(s, t)
            hit = self._forced[state] = tuple(out)
        return hit[:k]


def token_csr(token_bytes: Sequence[bytes]):
    """(tok_off int32 [V + 1], tok_dat uint8) of the token bytes"""
    lens = np.fromiter((len(b) for b in token_bytes), np.int64, len(token_bytes))
    off = np.zeros(len(token_bytes) + 1, np.int32)
    np.cumsum(lens, out=off[1:])
    dat = np.frombuffer(b"".join(token_bytes), np.uint8)
    return off, dat if len(dat) else np.zeros(1, np.uint8)


def _allow_table(dfa: np.ndarray, accept: np.ndarray, token_bytes: Sequence[bytes], eos_ids, csr=None) -> np.ndarray:
    """Pairs (state, token) that are still alive are carried as flat arrays, one byte position at a
    time: the first byte prunes most of S x V (a structural state admits a handful of bytes), the
    tokens are ordered by length so that only the still longer ones are touched, and the states
    are taken in blocks that bound the pair arrays."""
    S, V = dfa.shape[0], len(token_bytes)
    words = -(-V // 32)
    off, dat = csr if csr is not None else token_csr(token_bytes)
    off = off.astype(np.int64)
    lens = np.diff(off)
    toks = np.nonzero(lens > 0)[0]
    first = dat[off[toks]]
    by = np.argsort(first, kind="stable")
    toks_by_first = toks[by]
    g_cnt = np.bincount(first, minlength=256)
    g_start = np.concatenate([[0], np.cumsum(g_cnt)[:-1]])
    d32 = dfa.astype(np.int32)
    allow = np.zeros((S, words), np.uint32)
    per_state = ((d32 >= 0) * g_cnt[None, :]).sum(1)          # pairs alive after the first byte
    budget = 4_000_000
    s0 = 0
    while s0 < S:
        s1, tot = s0, 0
        while s1 < S and s1 - s0 < 256 and (s1 == s0 or tot + per_state[s1] <= budget):
            tot += per_state[s1]
            s1 += 1
        ss, bb = np.nonzero(d32[s0:s1] >= 0)
        cnt = g_cnt[bb]
        keep = cnt > 0
        ss, bb, cnt = ss[keep], bb[keep], cnt[keep]
        ok = np.zeros((s1 - s0, words * 32), bool)
        if len(ss):
            ends = np.cumsum(cnt)
            within = np.arange(ends[-1]) - np.repeat(ends - cnt, cnt)
            tok = toks_by_first[np.repeat(g_start[bb], cnt) + within]
            org = np.repeat(ss, cnt)
            st = np.repeat(d32[s0:s1][ss, bb], cnt)
            pos = 1
            while len(tok):
                done = lens[tok] == pos
                ok[org[done], tok[done]] = True
                go = ~done
                tok, org, st = tok[go], org[go], st[go]
                if not len(tok):
                    break
                st = d32[st, dat[off[tok] + pos]]
                live = st >= 0
                tok, org, st = tok[live], org[live], st[live]
                pos += 1
        allow[s0:s1] = np.packbits(ok, axis=1, bitorder="little").view("<u4")
        s0 = s1
    for t in eos_ids:
        t = int(t)
        if not 0 <= t < V:
            raise GuideError(f"eos id {t} is outside the vocabulary of {V} tokens")
        bit = np.uint32(1) << np.uint32(t & 31)
        allow[:, t >> 5] &= ~bit
        allow[accept, t >> 5] |= bit
    return allow.view(np.int32)


def compile_guide(kind: str, spec, token_bytes: Sequence[bytes], eos_ids: Sequence[int], csr=None) -> Guide:
    """Compile a guide of ``kind`` ("regex", "choice", "json_schema") for the vocabulary
    ``token_bytes`` (one ``bytes`` per id; empty for special or added tokens, which are never
    allowed) with the end-of-sequence ids ``eos_ids`` (allowed exactly in accepting states)."""
    text = lower(kind, spec)
    dfa, accept = compile_regex(text)
    allow = _allow_table(dfa, accept, token_bytes, eos_ids, csr)
    return Guide(kind, text, dfa, accept, allow, token_bytes, eos_ids)


# ------------------------------------------------------------------ tokenizers
def _gpt2_unicode_to_byte() -> dict:
    bs = list(range(33, 127)) + list(range(161, 173)) + list(range(174, 256))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {chr(c): b for b, c in zip(bs, cs)}


_TOK_CACHE: dict = {}
_TOK_LOCK = threading.Lock()


def _has_bytelevel(dec) -> bool:
    if not isinstance(dec, dict):
        return False
    if dec.get("type") == "ByteLevel":
        return True
    return dec.get("type") == "Sequence" and any(_has_bytelevel(d) for d in dec.get("decoders", []))


def token_bytes_of(tokenizer) -> list:
    """``list[bytes]`` per vocabulary id of a ``tokenizers.Tokenizer`` with a ByteLevel decoder
    (Qwen2, Llama-3, the synthetic packs): the inverse of the GPT-2 byte-to-unicode table.  Added
    and special tokens get no bytes.  Cached per tokenizer object."""
    key = id(tokenizer)
    with _TOK_LOCK:
        hit = _TOK_CACHE.get(key)
        if hit is not None and hit[0] is tokenizer:
            return hit[1]
    try:
        conf = json.loads(tokenizer.to_str())
        vocab = tokenizer.get_vocab(with_added_tokens=True)
        added = set(tokenizer.get_added_tokens_decoder())
    except Exception as e:  # noqa: BLE001 - not a tokenizers.Tokenizer
        raise GuideError(f"guided decoding is not supported for this model's tokenizer ({e})") from None
    if not _has_bytelevel(conf.get("decoder")):
        raise GuideError("guided decoding is not supported for this model: its tokenizer has no ByteLevel decoder")
    inv = _gpt2_unicode_to_byte()
    V = max(max(vocab.values(), default=-1), max(added, default=-1)) + 1
    out = [b""] * V
    for s, t in vocab.items():
        if t in added:
            continue
        try:
            out[t] = bytes(inv[c] for c in s)
        except KeyError:
            out[t] = b""            # not a byte-level string: never allowed
    with _TOK_LOCK:
        _TOK_CACHE[key] = (tokenizer, out)
    return out


# ------------------------------------------------------------------ cache of compiled guides
_GUIDES: "OrderedDict" = OrderedDict()
_GUIDES_LOCK = threading.Lock()
GUIDE_CACHE_SIZE = 64


def cached_guide(kind: str, spec, token_bytes: Sequence[bytes], eos_ids: Sequence[int], vocab_key=None) -> Guide:
    """:func:`compile_guide` behind an LRU keyed by (kind, spec text, vocabulary identity, eos ids).
    Runs in the caller's (the request's) thread."""
    text = spec if isinstance(spec, str) else json.dumps(spec, sort_keys=False, ensure_ascii=False)
    key = (kind, text, id(token_bytes) if vocab_key is None else vocab_key, tuple(sorted(int(t) for t in eos_ids)))
    with _GUIDES_LOCK:
        g = _GUIDES.get(key)
        if g is not None and (vocab_key is not None or g.token_bytes is token_bytes):
            _GUIDES.move_to_end(key)
            return g
    g = compile_guide(kind, spec, token_bytes, eos_ids)
    with _GUIDES_LOCK:
        _GUIDES[key] = g
        while len(_GUIDES) > GUIDE_CACHE_SIZE:
            _GUIDES.popitem(last=False)
    return g
