"""Guided requests through the engine's host sampling path (the CPU): the text of a guided request
matches its grammar and ends with ``stop``, alone and in a batch next to an unguided request, and
the VLM service accepts ``guided_choice`` / ``guided_regex`` / ``guided_json``."""
import json
import re

import numpy as np
import pytest
import torch

from lumen_amd.models.llm import LLM, LLM_PRESETS
from lumen_amd.runtime import guided as gd
from lumen_amd.runtime.engine import LLMEngine, SamplingParams
from lumen_amd.runtime.kv_cache import PagedKVCache

CFG = LLM_PRESETS["tiny"]
PATTERNS = [r"(yes|no|maybe)", r'\{"n": [0-9]{1,3}, "ok": (true|false)\}']
KINDS = {"greedy": {}, "sampled": dict(temperature=0.9, top_p=0.95, seed=11),
         "penalised": dict(temperature=0.8, repetition_penalty=1.3, seed=5)}


def vocab300():
    """300 ids: the 256 single bytes, multi-byte tokens, and two special ids without bytes (298 and
    299 = EOS); padded to the model's vocabulary with ids that are never allowed"""
    multi = ["true", "false", "null", ", ", '{"', '":', '": ', '"}', "yes", "no", "maybe", "ye", "may", "be",
             '"n"', '"ok"', "10", "42", "99", "00", "07", "123", "ab", "abc", "the", " a", "tru", "e}", "€", "日本"]
    tb = [bytes([i]) for i in range(256)] + [m.encode() for m in multi]
    tb += [bytes([97 + i % 26, 97 + i // 26]) for i in range(298 - len(tb))]
    return tb + [b"", b""]


EOS = 299
VOCAB = vocab300() + [b""] * (CFG.vocab_size - 300)
PROMPTS = [list(np.random.default_rng(i).integers(0, 256, 18 + 5 * i)) for i in range(4)]


@pytest.fixture(scope="module")
def engine():
    m = LLM(CFG, dtype=torch.float32, device="cpu")
    m.random_init(3)
    kv = PagedKVCache(CFG.num_layers, m.Hkv, CFG.head_dim, num_blocks=64, dtype=torch.float32)
    eng = LLMEngine(m, kv, lambda ids: m.embed_tokens(torch.tensor(ids)), max_batch=8)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def guides():
    return [gd.compile_guide("regex", p, VOCAB, [EOS]) for p in PATTERNS]


def _run(eng, jobs):
    rs = [eng.submit(p, len(p), SamplingParams(stop_token_ids=(EOS,), **kw)) for p, kw in jobs]
    for r in rs:
        list(r.stream(timeout=120))
    return rs


def _text(r) -> bytes:
    return b"".join(VOCAB[t] for t in r.tokens)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("which", [0, 1])
def test_guided_request_matches_and_stops(engine, guides, which, kind):
    r = _run(engine, [(PROMPTS[0], dict(max_new_tokens=40, guide=guides[which], **KINDS[kind]))])[0]
    assert re.fullmatch(PATTERNS[which], _text(r).decode()), _text(r)
    assert r.finish_reason == "stop" and EOS not in r.tokens


def test_batch_of_guided_requests_next_to_an_unguided_one(engine, guides):
    free = (PROMPTS[3], dict(max_new_tokens=14, temperature=0.7, seed=2))
    solo = _run(engine, [free])[0].tokens
    jobs = [(PROMPTS[0], dict(max_new_tokens=40, guide=guides[0])),
            (PROMPTS[1], dict(max_new_tokens=40, guide=guides[1], **KINDS["sampled"])),
            (PROMPTS[2], dict(max_new_tokens=40, guide=guides[1], **KINDS["penalised"])), free]
    rs = _run(engine, jobs)
    for r, which in zip(rs[:3], (0, 1, 1)):
        assert re.fullmatch(PATTERNS[which], _text(r).decode()), _text(r)
        assert r.finish_reason == "stop"
    assert len({len(r.tokens) for r in rs[:3]}) > 1, "the guided requests were to leave the batch at different steps"
    assert rs[3].tokens == solo and rs[3].finish_reason == "length"
    assert engine.stats["guided_steps"] == 0, "the CPU engine samples on the host"


def test_max_new_tokens_cuts_a_guided_request(engine, guides):
    g = guides[1]
    for n in (1, 2, 5):
        r = _run(engine, [(PROMPTS[1], dict(max_new_tokens=n, guide=g, **KINDS["sampled"]))])[0]
        assert r.finish_reason == "length" and len(r.tokens) == n
        s = g.start
        for k, t in enumerate(r.tokens):          # every emitted prefix is a prefix of some match
            s = g.walk(s, t)
            assert s >= 0, (k, _text(r))
        assert s == r.gstate and not re.fullmatch(PATTERNS[1], _text(r).decode())


def test_guided_requests_are_refused_under_tensor_parallelism(engine, guides):
    class FakeSync:
        pass

    engine.sync = FakeSync()
    try:
        with pytest.raises(ValueError, match="tensor parallelism"):
            engine.submit(PROMPTS[0], len(PROMPTS[0]), SamplingParams(max_new_tokens=4, guide=guides[0]))
    finally:
        engine.sync = None


# ------------------------------------------------------------------ service level
@pytest.fixture(scope="module")
def vlm_service(tmp_path_factory):
    from lumen_amd.models.vlm import write_vlm_model
    from lumen_amd.resources.validator import config_from_dict
    from lumen_amd.services.vlm import GeneralFastVLMService

    d = tmp_path_factory.mktemp("cache")
    write_vlm_model(d / "models" / "fastvlm-tiny", "fastvlm-tiny")
    cfg = {"metadata": {"version": "1.0.0", "region": "other", "cache_dir": str(d)},
           "deployment": {"mode": "single", "service": "vlm"}, "server": {"port": 50557, "host": "127.0.0.1"},
           "services": {"vlm": {"enabled": True, "package": "lumen_vlm",
                                "import_info": {"registry_class": "lumen_vlm.fastvlm.GeneralFastVLMService",
                                                "add_to_server": "lumen_vlm.proto.ml_service_pb2_grpc.add_InferenceServicer_to_server"},
                                "backend_settings": {"device": "cpu"},
                                "models": {"general": {"model": "fastvlm-tiny", "runtime": "onnx"}}}}}
    s = GeneralFastVLMService.from_config(config_from_dict(cfg).services["vlm"], d)
    s.initialize()
    yield s
    s.close()


def _img():
    from lumen_amd.utils.image import encode_jpeg

    return encode_jpeg(np.random.default_rng(0).integers(0, 255, (40, 60, 3), dtype=np.uint8))


def test_service_guided_choice(vlm_service):
    choices = ["indoor", "outdoor", "unclear"]
    body, _, meta = vlm_service.handle("vlm_generate", _img(), "image/jpeg",
                                       {"prompt": "Where?", "max_new_tokens": "32", "guided_choice": json.dumps(choices)})
    d = json.loads(body)
    assert d["text"] in choices and d["finish_reason"] == "stop"
    assert meta["guided"] == "choice" and meta["finish_reason"] == "stop"
    body, _, meta = vlm_service.handle("vlm_generate", _img(), "image/jpeg",
                                       {"prompt": "When?", "max_new_tokens": "32", "temperature": "0.8", "seed": "4",
                                        "guided_regex": r"\d{4}-\d{2}-\d{2}"})
    assert re.fullmatch(r"\d{4}-\d{2}-\d{2}", json.loads(body)["text"]) and meta["guided"] == "regex"
    schema = {"type": "object", "properties": {"ok": {"type": "boolean"}, "n": {"type": "integer"}}}
    body, _, meta = vlm_service.handle("vlm_generate", _img(), "image/jpeg",
                                       {"prompt": "Tag.", "max_new_tokens": "64", "guided_json": json.dumps(schema)})
    d = json.loads(body)
    if d["finish_reason"] == "stop":              # an integer has no length bound: the cut is legitimate
        v = json.loads(d["text"])
        assert list(v) == ["ok", "n"] and isinstance(v["ok"], bool) and isinstance(v["n"], int)
    assert meta["guided"] == "json_schema"


def test_service_guided_stream_and_capability(vlm_service):
    from lumen_amd.proto import ml_service as pb

    req = pb.InferRequest(correlation_id="g1", task="vlm_generate_stream", payload=_img(), payload_mime="image/jpeg",
                          meta={"prompt": "Hi", "max_new_tokens": "16", "guided_choice": '["alpha", "beta"]'})
    out = list(vlm_service.Infer(iter([req]), None))
    assert out[-1].is_final and json.loads(out[-1].result)["text"] in ("alpha", "beta")
    assert out[-1].meta["guided"] == "choice"
    cap = vlm_service.build_capability()
    assert json.loads(cap.extra["guided_decoding"]) == ["choice", "regex", "json_schema"]


def test_service_rejects_bad_guides(vlm_service):
    from lumen_amd.services.vlm.backend import InvalidInputError

    base = {"prompt": "x", "max_new_tokens": "4"}
    for extra, msg in [({"guided_choice": '["a"]', "guided_regex": "a"}, "At most one"),
                       ({"guided_regex": "a(?=b)"}, "look-around"),
                       ({"guided_regex": "(a"}, "offset"),
                       ({"guided_choice": "[1,"}, "malformed JSON"),
                       ({"guided_json": '{"type": "string", "format": "date"}'}, "format")]:
        with pytest.raises(InvalidInputError, match=msg):
            vlm_service.handle("vlm_generate", _img(), "image/jpeg", {**base, **extra})
    # unguided requests are untouched
    body, _, meta = vlm_service.handle("vlm_generate", _img(), "image/jpeg", base)
    assert json.loads(body)["generated_tokens"] == 4 and "guided" not in meta
