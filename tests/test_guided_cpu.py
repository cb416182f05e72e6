"""Guided decoding on the CPU: the regex compiler against Python's ``re``, the token tables against
an independent byte walk, JSON-schema guides under random constrained generation, and the CPU
reference of ``sample_rows(guide=...)`` against masking the logits by hand."""
import json
import re
from collections import deque

import numpy as np
import pytest
import torch

from lumen_amd.ops import llm as lops
from lumen_amd.runtime import guided as gd

# every supported construct: literals, '.', classes and negated classes with ranges, the class
# escapes and their negations, escaped metacharacters, groups, alternation, * + ?, {m} {m,} {m,n},
# non-ASCII literals and classes.  Each has far more than 100 distinct matches.
PATTERNS = [
    r"[a-z]+@[a-z]+\.(com|org)",
    r"\d{4}-\d{2}-\d{2}",
    r"(yes|no|maybe)( (yes|no|maybe)){0,4}",
    r'\{"n": [0-9]{1,3}, "ok": (true|false)\}',
    r"[^a-c]x.{0,2}",
    r"[α-ωé]+!?",
    r"(ab)*[c-f]+|d{2,}[xy]*",
    r"\w+\s\S\W",
    r"-?(0|[1-9][0-9]*)(\.[0-9]+)?",
    r'"([^"\\]|\\["\\/bfnrt])*"',
    r"[\d\-+]{3,5}",
    r"[ab]{2}b{2,}[cd]{1,3}x*",
    r"(?:x|yz|[0-9])+\t\r\n",
    r"[^\n\x00-\x1f]{1,3}",
    r"héllo wörld [0-9]+",
    r'\.\*\+\?\(\)\[\]\{\}\|\\\/\"[a-z]{2,3}',
    r".*end",
    r"([A-Z][a-z]*)( [A-Z][a-z]*)*",
    r"[日本語]{2,4}k?",
    r"\D\d\S\s\W\w{0,2}",
]


def _accepts(dfa, accept, data: bytes) -> bool:
    s = 0
    for b in data:
        s = int(dfa[s, b])
        if s < 0:
            return False
    return bool(accept[s])


def _dist_to_accept(dfa, accept):
    S = dfa.shape[0]
    dist = np.where(accept, 0, -1)
    rev = [[] for _ in range(S)]
    for s in range(S):
        for t in set(int(x) for x in dfa[s] if x >= 0):
            rev[t].append(s)
    q = deque(np.nonzero(accept)[0].tolist())
    while q:
        t = q.popleft()
        for s in rev[t]:
            if dist[s] < 0:
                dist[s] = dist[t] + 1
                q.append(s)
    return dist


def _walks(dfa, accept, rng, n, free=30):
    """random walks of the DFA from the start to an accepting state: ``free`` random live steps
    at most (stopping early in an accepting state now and then), then downhill to the nearest one"""
    dist = _dist_to_accept(dfa, accept)
    assert (dist >= 0).all(), "a state without a way to finish"
    out = set()
    for _ in range(n):
        s, data = 0, bytearray()
        for _ in range(int(rng.integers(0, free + 1))):
            if accept[s] and rng.random() < 0.3:
                break
            live = np.nonzero(dfa[s] >= 0)[0]
            if not len(live):
                break
            b = int(rng.choice(live))
            data.append(b)
            s = int(dfa[s, b])
        while not accept[s]:
            live = [b for b in np.nonzero(dfa[s] >= 0)[0] if dist[dfa[s, b]] < dist[s]]
            b = int(rng.choice(live))
            data.append(b)
            s = int(dfa[s, b])
        out.add(bytes(data))
    return out


def _re_accepts(pat, data: bytes) -> bool:
    """``re.fullmatch`` on the decoded text; bytes that are not UTF-8 are no string at all"""
    try:
        text = data.decode("utf-8")
    except UnicodeDecodeError:
        return False
    return re.fullmatch(pat, text, re.ASCII) is not None


@pytest.mark.parametrize("pat", PATTERNS)
def test_regex_agrees_with_re(pat):
    dfa, accept = gd.compile_regex(pat)
    rng = np.random.default_rng(len(pat))
    pos = _walks(dfa, accept, rng, 600)
    assert len(pos) >= 100, f"only {len(pos)} distinct positives: pick another pattern"
    neg_text, neg_raw = set(), set()
    for p in sorted(pos):
        for k in range(8):
            m = bytearray(p)
            kind = int(rng.integers(0, 3)) if m else 1
            at = int(rng.integers(0, len(m) + (kind == 1))) if m else 0
            byte = int(rng.integers(0, 256)) if k % 2 else int(rng.integers(32, 127))   # any byte, or printable ASCII
            if kind == 0:
                m[at] = byte
            elif kind == 1:
                m.insert(at, byte)
            else:
                del m[at]
            m = bytes(m)
            if _re_accepts(pat, m):
                continue
            try:
                m.decode("utf-8")
                neg_text.add(m)
            except UnicodeDecodeError:
                neg_raw.add(m)
    assert len(neg_text) >= 100, f"only {len(neg_text)} decodable negatives: pick another pattern"
    for p in pos:
        assert _re_accepts(pat, p), (pat, p)                      # what the DFA accepts, re accepts
    for m in neg_text | neg_raw:
        assert not _accepts(dfa, accept, m), (pat, m)             # what re rejects, the DFA rejects
    # and the other direction on the mutations re accepts
    for p in list(pos)[:200]:
        m = bytearray(p)
        if m:
            m[int(rng.integers(0, len(m)))] = int(rng.integers(32, 127))
        assert _accepts(dfa, accept, bytes(m)) == _re_accepts(pat, bytes(m)), (pat, bytes(m))


@pytest.mark.parametrize("pat,what", [(r"a(?=b)", "look-around"), (r"a(?<!b)", "look-around"), (r"(a)\1", "back-ref"),
                                      (r"a*?", "lazy"), (r"a+?b", "lazy"), (r"^ab", "anchor"), (r"ab$", "anchor"),
                                      (r"a\b", "escape"), (r"(?i)a", "flags"), (r"(ab", "missing"), (r"[ab", "missing"),
                                      (r"*a", "repeat")])
def test_unsupported_syntax_raises_with_the_offset(pat, what):
    with pytest.raises(gd.GuideError, match=r"at offset \d+"):
        gd.compile_regex(pat)


def test_state_cap(monkeypatch):
    monkeypatch.setenv("LUMEN_GUIDED_MAX_STATES", "16")
    with pytest.raises(gd.GuideError, match="LUMEN_GUIDED_MAX_STATES"):
        gd.compile_regex(r"[a-z]{40}")
    monkeypatch.delenv("LUMEN_GUIDED_MAX_STATES")
    assert gd.compile_regex(r"[a-z]{40}")[0].shape[0] == 41


# ------------------------------------------------------------------ token tables
def vocab300():
    """300 ids: the 256 single bytes, multi-byte tokens (among them a 3-byte UTF-8 character whose
    first two bytes are one token -- the third is the single byte 0xAC), two special ids without
    bytes: 298 (padding) and 299 (EOS)"""
    multi = ["true", "false", "null", ", ", '{"', '":', '": ', '"}', "yes", "no", "maybe", "ye", "s", "may", "be",
             '"n"', '"ok"', "10", "42", "99", "00", "07", "123", "ab", "abc", "the", " a", "\n\n", "tru", "e}", "€",
             "日本", "é", "[]", '["', '"]', '", "', "-1", "0.5", "e+", "}}"]
    tb = [bytes([i]) for i in range(256)] + [m.encode() for m in multi]
    tb[256 + multi.index("s")] = "€".encode()[:2]           # the split character's head
    tb += [bytes([97 + i % 26, 97 + i // 26]) for i in range(298 - len(tb))]
    tb += [b"", b""]
    assert len(tb) == 300
    return tb


VOCAB, PAD, EOS = vocab300(), 298, 299
TABLE_PATTERNS = [PATTERNS[2], PATTERNS[3], r"[€a-c]{1,3}(true|false)", PATTERNS[9], r".{0,3}"]


@pytest.mark.parametrize("pat", TABLE_PATTERNS)
def test_token_tables_equal_the_byte_walk(pat):
    g = gd.compile_guide("regex", pat, VOCAB, [EOS])
    S, V = g.n_states, len(VOCAB)
    assert g.dfa.dtype == np.int16 and g.allow.dtype == np.int32 and g.allow.shape == (S, -(-V // 32))
    assert g.start == 0 and g.accept.shape == (S,)
    bits = (g.allow.view(np.uint32)[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    bits = bits.reshape(S, -1).astype(bool)
    assert not bits[:, V:].any(), "bits at or beyond V"
    for s in range(S):
        for t, data in enumerate(VOCAB):
            cur = s                                      # the independent byte walk
            for b in data:
                cur = int(g.dfa[cur, b])
                if cur < 0:
                    break
            want = len(data) > 0 and cur >= 0
            if t == EOS:
                want = bool(g.accept[s])
            assert bits[s, t] == want, (s, t, data)
            assert g.allows(s, t) == want
            if t == EOS or not data:
                assert g.walk(s, t) == s                 # EOS and empty tokens leave the state
            else:
                assert g.walk(s, t) == (cur if cur >= 0 else -1)
        assert bits[s].any(), f"state {s} allows nothing"
    assert not bits[:, PAD].any()
    assert (bits[:, EOS] == g.accept).all()


def test_split_utf8_character_is_reachable_through_two_tokens():
    g = gd.compile_guide("regex", r"[€a-c]{1,3}(true|false)", VOCAB, [EOS])
    head = VOCAB.index("€".encode()[:2])
    assert g.allows(0, head) and g.allows(0, VOCAB.index("€".encode()))
    mid = g.walk(0, head)
    assert g.allows(mid, 0xAC) and not g.allows(mid, ord("a")), "only the continuation byte may follow"
    assert g.walk(mid, 0xAC) == g.walk(0, VOCAB.index("€".encode()))


def test_choice_and_cache():
    g = gd.cached_guide("choice", ["yes", "no", "a.b|c"], VOCAB, [EOS])
    assert gd.cached_guide("choice", ["yes", "no", "a.b|c"], VOCAB, [EOS]) is g
    for text in ("yes", "no", "a.b|c"):
        assert _accepts(g.dfa, g.accept, text.encode())
    assert not _accepts(g.dfa, g.accept, b"axb|c") and not _accepts(g.dfa, g.accept, b"ye")
    with pytest.raises(gd.GuideError):
        gd.compile_guide("choice", "[1, 2]", VOCAB, [EOS])
    with pytest.raises(gd.GuideError, match="malformed JSON"):
        gd.compile_guide("choice", "[", VOCAB, [EOS])


def test_token_bytes_of_a_bytelevel_tokenizer(tmp_path):
    from tokenizers import Tokenizer, models

    from lumen_amd.resources.synthetic import write_byte_bpe_tokenizer

    info = write_byte_bpe_tokenizer(tmp_path / "tokenizer.json", extra_special=["<image>"], fill_vocab=300)
    tok = Tokenizer.from_file(str(tmp_path / "tokenizer.json"))
    tb = gd.token_bytes_of(tok)
    assert gd.token_bytes_of(tok) is tb, "cached per tokenizer object"
    assert len(tb) == 300 and tb[:256] == [bytes([i]) for i in range(256)]
    assert tb[info["eos_id"]] == b"" and tb[info["bos_id"]] == b"" and tb[299] == b" w" + str(299 - 259).encode()
    with pytest.raises(gd.GuideError, match="not supported for this model"):
        gd.token_bytes_of(Tokenizer(models.WordLevel(vocab={"a": 0, "[UNK]": 1}, unk_token="[UNK]")))


# ------------------------------------------------------------------ JSON schema
PHOTO = {"type": "object",
         "properties": {"caption": {"type": "string", "maxLength": 10},
                        "tags": {"type": "array", "items": {"type": "string", "maxLength": 4}, "maxItems": 2},
                        "nsfw": {"type": "boolean"},
                        "people": {"type": "integer"}},
         "required": ["caption", "tags", "nsfw", "people"]}
SMALL = [{"type": "object", "properties": {"ok": {"type": "boolean"}, "skipped": {"type": "null"},
                                           "label": {"enum": ["cat", "dog", 3]}}, "required": ["ok", "label"]},
         {"type": "array", "items": {"anyOf": [{"type": "number"}, {"type": "null"}]}, "minItems": 1, "maxItems": 3},
         {"type": "object", "properties": {"id": {"type": "string", "pattern": "[a-f0-9]{4}"},
                                           "pos": {"type": "object", "properties": {"x": {"type": "integer"},
                                                                                    "note": {"type": "string",
                                                                                             "maxLength": 3}}}}}]


def _check(schema, v):
    """the value has the schema's keys and types (by hand: the subset the test schemas use)"""
    if "enum" in schema:
        assert v in schema["enum"] and type(v) in {type(e) for e in schema["enum"]}
        return
    if "anyOf" in schema:
        errs = []
        for s in schema["anyOf"]:
            try:
                _check(s, v)
                return
            except AssertionError as e:
                errs.append(e)
        raise AssertionError(f"{v!r} matches no branch")
    ty = schema["type"]
    if ty == "object":
        want = [k for k in schema["properties"] if "required" not in schema or k in schema["required"]]
        assert isinstance(v, dict) and list(v) == want, (v, want)
        for k in want:
            _check(schema["properties"][k], v[k])
    elif ty == "array":
        assert isinstance(v, list) and schema.get("minItems", 0) <= len(v) <= schema.get("maxItems", 10 ** 9)
        for x in v:
            _check(schema["items"], x)
    elif ty == "string":
        assert isinstance(v, str) and len(v) <= schema.get("maxLength", 10 ** 9)
        if "pattern" in schema:
            assert re.fullmatch(schema["pattern"], v)
    elif ty == "integer":
        assert isinstance(v, int) and not isinstance(v, bool)
    elif ty == "number":
        assert isinstance(v, (int, float)) and not isinstance(v, bool)
    elif ty == "boolean":
        assert isinstance(v, bool)
    else:
        assert ty == "null" and v is None


@pytest.mark.parametrize("schema", [PHOTO] + SMALL, ids=["photo", "flags", "numbers", "nested"])
def test_json_schema_random_generation(schema):
    g = gd.compile_guide("json_schema", json.dumps(schema), VOCAB, [EOS])
    rng = np.random.default_rng(7)
    allowed = [np.nonzero((g.allow.view(np.uint32)[s][:, None] >> np.arange(32, dtype=np.uint32)).reshape(-1) & 1)[0]
               for s in range(g.n_states)]
    ended = 0
    for _ in range(200):
        s, out = g.start, bytearray()
        for _ in range(200):
            t = int(rng.choice(allowed[s]))
            if t == EOS:
                ended += 1
                text = out.decode("utf-8")          # a match is well-formed UTF-8
                _check(schema, json.loads(text))
                break
            out += VOCAB[t]
            s = g.walk(s, t)
            assert s >= 0
    assert ended >= 100, f"only {ended} of 200 generations ended by EOS: bound the schema's lengths"


@pytest.mark.parametrize("schema,kw", [({"type": "string", "format": "date"}, "format"),
                                       ({"type": "integer", "minimum": 0}, "minimum"),
                                       ({"$ref": "#/defs/x"}, r"\$ref"),
                                       ({"type": "object", "properties": {}, "patternProperties": {}}, "patternProperties"),
                                       ({"type": "object", "properties": {}, "additionalProperties": True},
                                        "additionalProperties"),
                                       ({"oneOf": [{"type": "null"}]}, "oneOf"),
                                       ({"type": "array", "items": {"type": "null"}, "uniqueItems": True}, "uniqueItems")])
def test_unsupported_keywords_raise_naming_the_keyword(schema, kw):
    with pytest.raises(gd.GuideError, match=kw):
        gd.compile_guide("json_schema", schema, VOCAB, [EOS])


def test_over_cap_schema_raises(monkeypatch):
    monkeypatch.setenv("LUMEN_GUIDED_MAX_STATES", "64")
    with pytest.raises(gd.GuideError, match="LUMEN_GUIDED_MAX_STATES"):
        gd.compile_guide("json_schema", PHOTO, VOCAB, [EOS])


# ------------------------------------------------------------------ the CPU reference of sample_rows(guide=...)
def _hand_guide(V, sets):
    """GuideTensors over the 300-id vocabulary padded to V: state a allows exactly ``sets[a]``; the
    transitions lead every byte to state (a + 1) % A, so the walk is checked too"""
    A = len(sets)
    allow = np.zeros((A, lops.seen_words(V)), np.uint32)
    for a, ts in enumerate(sets):
        for t in ts:
            allow[a, t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    dfa = np.tile(((np.arange(A) + 1) % A).astype(np.int16)[:, None], (1, 256))
    off, dat = gd.token_csr(VOCAB + [b""] * (V - len(VOCAB)))
    return allow, dfa, off, dat


def test_cpu_reference_equals_masking_by_hand():
    V, B = 512, 4
    rng = np.random.default_rng(0)
    logits = torch.from_numpy(rng.permutation(np.linspace(-9, 9, B * V)).astype(np.float32).reshape(B, V))
    order = logits.argsort(dim=1, descending=True)
    sets = [{int(order[0, 5])}, set(int(t) for t in order[1, [0, 3, 200, 400, 511]]),
            set(int(t) for t in rng.choice(V, 64, replace=False)), set(int(t) for t in rng.choice(V, V // 2, replace=False))]
    allow, dfa, off, dat = _hand_guide(V, sets)
    inv_t, top_p, pen = [1.0, 1 / 0.8, 1 / 0.7, 1 / 1.2], [1.0, 0.9, 0.95, 1.0], [1.3, 1.2, 1.0, 1.25]
    u, greedy, slot = [0.0, 0.35, 0.8, 0.6], [1, 0, 0, 0], [0, 1, -1, 2]
    in_ids = [int(order[b, 1]) for b in range(B)]
    seen = torch.zeros((3, lops.seen_words(V)), dtype=torch.int32)
    for b, sl in enumerate(slot):                   # seen bits that overlap the allowed sets
        for t in list(sets[b])[:3]:
            if sl >= 0:
                lops._mark_seen(seen, sl, t)
    guide = lops.GuideTensors(torch.from_numpy(allow.view(np.int32)), torch.from_numpy(dfa), torch.from_numpy(off),
                              torch.from_numpy(dat.copy()), [0, 1, 2, 3], [0, 1, -1, 3],
                              torch.tensor([7, 7, 2, 7], dtype=torch.int32))
    v, i, lse, tok, seen2, state = lops.sample_rows(logits, inv_t, top_p, pen, u, greedy, slot, seen.clone(), in_ids,
                                                    guide=guide)
    masked = logits.clone()
    for b in range(B):
        keep = torch.zeros(V, dtype=torch.bool)
        keep[list(sets[b])] = True
        masked[b, ~keep] = float("-inf")
    rv, ri, rlse, rtok, rseen = lops.sample_rows(masked, inv_t, top_p, pen, u, greedy, slot, seen.clone(), in_ids)
    assert torch.equal(v.view(torch.int32), rv.view(torch.int32)) and torch.equal(i, ri)
    assert torch.equal(lse.view(torch.int32), rlse.view(torch.int32))
    assert torch.equal(tok, rtok) and torch.equal(seen2, rseen)
    assert all(int(tok[b]) in sets[b] for b in range(B))
    assert int(tok[0]) == int(order[0, 5]) and bool(torch.isinf(v[0, 1:]).all())      # one allowed: the tail is -inf
    # the walk: every token with bytes moves state a to a + 1 (mod 4); row 2 read its state from the array
    has_bytes = [int(t) < 300 and len(VOCAB[int(t)]) > 0 for t in tok]
    assert state.tolist() == [(b + 1) % 4 if has_bytes[b] else b for b in range(4)]     # row b drew in state b


def test_cpu_reference_nothing_allowed_and_mask_logits():
    V = 512
    logits = torch.randn(2, V, generator=torch.Generator().manual_seed(1))
    allow, dfa, off, dat = _hand_guide(V, [{3, 40, 511}, set()])
    guide = lops.GuideTensors(torch.from_numpy(allow.view(np.int32)), torch.from_numpy(dfa), torch.from_numpy(off),
                              torch.from_numpy(dat.copy()), [0, -1], [-1, -1], torch.tensor([1], dtype=torch.int32))
    seen = torch.zeros((1, lops.seen_words(V)), dtype=torch.int32)
    out_ids = torch.full((2,), -7, dtype=torch.long)
    v, i, lse, tok, _, state = lops.sample_rows(logits, [1.0] * 2, [1.0] * 2, [1.0] * 2, [0.5] * 2, [0, 1], [-1] * 2, seen,
                                                [1, 1], out_ids=out_ids, guide=guide)
    assert int(tok[0]) == -1 and int(state[0]) == 1 and int(out_ids[0]) == 0, "nothing allowed: -1, state unchanged"
    assert int(tok[1]) == int(logits[1].argmax()), "g_slot = -1: an unguided row"
    x = logits.clone()
    lops.mask_logits_(x, [allow.view(np.int32)[0], None])
    assert torch.equal(x[1], logits[1])
    assert sorted(torch.isfinite(x[0]).nonzero().reshape(-1).tolist()) == [3, 40, 511]
    y = logits[:, 32:64].clone()                        # a vocabulary shard starting at column 32
    lops.mask_logits_(y, [allow.view(np.int32)[0][:2], None], v0=32)
    assert torch.isfinite(y[0]).nonzero().reshape(-1).tolist() == [8]
