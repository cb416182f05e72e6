"""Prefix KV caching on the CPU: the block manager's prefix index (publish / match / LRU
eviction), the engine's reuse of matched blocks (exact token equality against cold runs, fp32),
the VLM key builder and the service path on the synthetic tiny VLM pack."""
import json

import numpy as np
import pytest
import torch

from lumen_amd.models.llm import LLM, LLM_PRESETS
from lumen_amd.runtime.engine import LLMEngine, SamplingParams
from lumen_amd.runtime.kv_cache import BlockManager, PagedKVCache
from lumen_amd.services.vlm.backend import prefix_cache_keys


def _keys(n, seed=0):
    return np.random.default_rng(seed).integers(1, 2 ** 63, (n, 2), dtype=np.uint64)


# ----------------------------------------------------------------------------- block manager
def test_publish_match_longest_run_and_refcounts():
    bm = BlockManager(16)
    k = _keys(4)
    assert bm.reserve(1, 4 * 64 + 10)              # 5 blocks, 4 of them full
    t1 = bm.table(1)
    assert bm.publish(1, k) == 4
    assert bm.publish(1, k) == 0                   # already there
    assert bm.free_blocks() == 11 and bm.cached_blocks() == 0    # held by the sequence too
    # the whole run
    assert bm.match(k, 2) == 256 and bm.table(2) == t1[:4]
    # longest LEADING run: a miss in the middle ends it, later keys do not count
    bad = k.copy()
    bad[2] = (7, 7)
    assert bm.match(bad, 3) == 128 and bm.table(3) == t1[:2]
    # nothing matches: no sequence created
    assert bm.match(_keys(3, seed=9), 4) == 0
    with pytest.raises(KeyError):
        bm.table(4)
    assert bm.num_seqs() == 3
    # releases: blocks stay while anyone (or the index) holds them
    bm.release(1)
    assert bm.free_blocks() == 12 and bm.cached_blocks() == 0    # the partial block came back; 2 and 3 hold the rest
    bm.release(2)
    assert bm.cached_blocks() == 2 and bm.free_blocks() == 14    # blocks 2, 3 of the chain: index only
    bm.release(3)
    assert bm.cached_blocks() == 4 and bm.free_blocks() == 16 and bm.num_seqs() == 0
    # still matchable after every sequence is gone
    assert bm.match(k, 5) == 256 and bm.table(5) == t1[:4]
    assert bm.cached_blocks() == 0 and bm.free_blocks() == 12
    # a key that is already present keeps its block: another sequence publishing the same keys adds nothing
    assert bm.reserve(6, 128)
    assert bm.publish(6, k[:2]) == 0
    bm.release(6)
    assert bm.free_blocks() == 12
    with pytest.raises(KeyError):
        bm.publish(5, _keys(5, seed=3))            # more keys than full blocks
    with pytest.raises(KeyError):
        bm.publish(99, k)


def test_accounting_and_lru_eviction_deepest_first():
    bm = BlockManager(8)
    ka, kb = _keys(3, seed=1), _keys(3, seed=2)
    for seq, k in ((1, ka), (2, kb)):
        assert bm.reserve(seq, 192)
        assert bm.publish(seq, k) == 3
        bm.release(seq)
    assert bm.cached_blocks() == 6 and bm.free_blocks() == 8
    assert bm.can_reserve(10, 8 * 64) and not bm.can_reserve(10, 8 * 64 + 1)
    # touch chain A: B is now the least recently matched
    assert bm.match(ka, 3) == 192
    bm.release(3)
    assert bm.cached_blocks() == 6
    # 2 free blocks + 1 eviction: B's deepest block goes first
    assert bm.reserve(10, 3 * 64)
    assert bm.cached_blocks() == 5 and bm.free_blocks() == 5
    assert bm.match(kb, 11) == 128
    bm.release(11)                                  # (this touched B's first two blocks: A is older now)
    assert bm.match(ka, 12) == 192                  # A untouched by the eviction
    bm.release(12)
    # evict two more: B's remaining blocks were matched before A's last match
    assert bm.reserve(10, 5 * 64)
    assert bm.cached_blocks() == 3
    assert bm.match(kb, 13) == 0
    assert bm.match(ka, 14) == 192
    # chain A is in use by a live sequence: never evicted, the pool is simply full
    assert bm.free_blocks() == 0 and bm.cached_blocks() == 0
    assert not bm.can_reserve(15, 64) and not bm.reserve(15, 64)
    t = bm.table(14)
    bm.release(10)
    assert bm.reserve(15, 5 * 64) and not set(bm.table(15)) & set(t)
    bm.release(14)
    bm.release(15)
    assert bm.free_blocks() == 8 and bm.cached_blocks() == 3 and bm.num_seqs() == 0


def test_never_publishing_sequences_see_the_old_behaviour():
    bm = BlockManager(6)
    assert bm.reserve(1, 130) and len(bm.table(1)) == 3 and bm.free_blocks() == 3
    assert bm.reserve(1, 190) and len(bm.table(1)) == 3
    assert not bm.reserve(2, 4 * 64) and bm.num_seqs() == 1
    assert bm.fork(1, 2) == 128 and bm.table(2) == bm.table(1)[:2]
    bm.release(1)
    assert bm.free_blocks() == 4
    bm.release(2)
    assert bm.free_blocks() == 6 and bm.cached_blocks() == 0 and bm.num_seqs() == 0
    assert bm.match(_keys(2), 3) == 0


# ----------------------------------------------------------------------------- engine (tiny, fp32)
CFG = LLM_PRESETS["tiny"]


@pytest.fixture(scope="module")
def llm():
    m = LLM(CFG, dtype=torch.float32, device="cpu")
    m.random_init(11)
    return m


def _engine(m, blocks=64, **kw):
    kv = PagedKVCache(CFG.num_layers, m.Hkv, CFG.head_dim, num_blocks=blocks, dtype=torch.float32)
    return LLMEngine(m, kv, lambda ids: m.embed_tokens(torch.tensor(ids)), max_batch=8, **kw), kv


def _prompts():
    rng = np.random.default_rng(5)
    prefix = [int(t) for t in rng.integers(0, CFG.vocab_size, 130)]
    return [prefix + [int(t) for t in rng.integers(0, CFG.vocab_size, n)] for n in (20, 45, 70, 1)]


def _pk(ids):
    return prefix_cache_keys(ids, [], b"")


def _run(eng, prompts, keys, new=10):
    rs = [eng.submit(p, len(p), SamplingParams(max_new_tokens=new), prefix_keys=_pk(p) if keys else None)
          for p in prompts]
    for r in rs:
        list(r.stream(timeout=120))
    return rs


@pytest.fixture(scope="module")
def cold(llm):
    eng, kv = _engine(llm)
    try:
        rs = _run(eng, _prompts(), keys=False)
        assert all(r.cached_tokens == 0 for r in rs) and kv.blocks.cached_blocks() == 0
        assert eng.stats["prefix_hits"] == 0 and eng.stats["prefill_tokens"] == sum(len(p) for p in _prompts())
        return [list(r.tokens) for r in rs]
    finally:
        eng.close()


def test_engine_hits_equal_cold_runs(llm, cold):
    eng, kv = _engine(llm)
    try:
        ps = _prompts()
        got = []
        for p in ps:                                # one after the other: every later prompt hits
            got += _run(eng, [p], keys=True)
        assert [r.cached_tokens for r in got] == [0, 128, 128, 128]
        assert [list(r.tokens) for r in got] == cold
        assert eng.stats["prefix_hits"] == 3 and eng.stats["prefix_tokens"] == 3 * 128
        assert eng.stats["prefill_tokens"] == sum(len(p) for p in ps) - 3 * 128
        assert kv.blocks.num_seqs() == 0 and kv.blocks.cached_blocks() > 0
        assert kv.blocks.free_blocks() == 64
    finally:
        eng.close()


def test_engine_hits_under_concurrent_submission(llm, cold):
    eng, kv = _engine(llm)
    try:
        ps = _prompts()
        first = _run(eng, ps[:1], keys=True)
        rest = _run(eng, ps[1:], keys=True)         # submitted together, all forked from the first
        assert [r.cached_tokens for r in rest] == [128, 128, 128]
        assert [list(r.tokens) for r in first + rest] == cold
        # all at once on a fresh index: whoever hits or misses, the tokens are the cold ones
        eng2, _ = _engine(llm)
        try:
            assert [list(r.tokens) for r in _run(eng2, ps, keys=True)] == cold
        finally:
            eng2.close()
    finally:
        eng.close()


def test_engine_eviction_while_a_forked_request_runs(llm):
    ps = _prompts()
    rng = np.random.default_rng(77)
    others = [[int(t) for t in rng.integers(0, CFG.vocab_size, 150)] for _ in range(2)]
    eng, _ = _engine(llm)
    try:
        want = list(_run(eng, [ps[1]], keys=False, new=200)[0].tokens)
        want_o = [list(r.tokens) for r in _run(eng, others, keys=False)]
    finally:
        eng.close()
    eng, kv = _engine(llm, blocks=10)
    try:
        _run(eng, [ps[0]], keys=True)               # publishes the two prefix blocks
        assert kv.blocks.cached_blocks() == 2
        b = eng.submit(ps[1], len(ps[1]), SamplingParams(max_new_tokens=200), prefix_keys=_pk(ps[1]))
        # 6 of 10 blocks are b's (two of them shared); each other prompt needs 3 and publishes 2:
        # the second one can only be admitted by evicting a block the first one left in the index
        got_o = []
        for o in others:
            got_o.append(list(_run(eng, [o], keys=True)[0].tokens))
            assert b.finish_reason is None, "the forked request should still be running"
        assert kv.blocks.match(_pk(others[0]), 1 << 40) < 128       # evicted (deepest block first)
        kv.blocks.release(1 << 40)
        list(b.stream(timeout=300))
        assert b.cached_tokens == 128 and list(b.tokens) == want and got_o == want_o
    finally:
        eng.close()


class _NullSync:
    """stands in for the TP step channel: the leader's sends go nowhere"""

    def send(self, msg):
        pass

    def send_decode(self, *a, **k):
        pass

    def close(self):
        pass


def test_engine_tp_sync_ignores_keys(llm, cold):
    eng, kv = _engine(llm, tp_sync=_NullSync())
    try:
        ps = _prompts()
        rs = []
        for p in ps[:2]:
            rs += _run(eng, [p], keys=True)
        assert [r.cached_tokens for r in rs] == [0, 0] and [list(r.tokens) for r in rs] == cold[:2]
        assert eng.stats["prefix_hits"] == 0 and kv.blocks.cached_blocks() == 0
        hit = eng.match_prefix(_pk(ps[0]), len(ps[0]))
        assert hit.tokens == 0
    finally:
        eng.close()


def test_engine_hit_is_capped_below_the_last_row(llm):
    rng = np.random.default_rng(3)
    p128 = [int(t) for t in rng.integers(0, CFG.vocab_size, 128)]
    p129 = p128 + [5]
    eng, kv = _engine(llm)
    try:
        a = _run(eng, [p128], keys=True)[0]
        b = _run(eng, [p128], keys=True)[0]          # both blocks are cached, the last row still runs
        assert (a.cached_tokens, b.cached_tokens) == (0, 64) and list(a.tokens) == list(b.tokens)
        c = _run(eng, [p129], keys=True)[0]
        assert c.cached_tokens == 128
        # a hit taken without the prompt length is cut back at submit
        hit = eng.match_prefix(_pk(p128))
        assert hit.tokens == 128
        d = eng.submit(p128, 128, SamplingParams(max_new_tokens=10), prefix_keys=_pk(p128), hit=hit)
        list(d.stream(timeout=120))
        assert d.cached_tokens == 64 and list(d.tokens) == list(a.tokens)
        # an abandoned hit gives its references back
        hit = eng.match_prefix(_pk(p129), 129)
        assert hit.tokens == 128 and kv.blocks.num_seqs() == 1
        eng.release_prefix(hit)
        assert kv.blocks.num_seqs() == 0 and kv.blocks.free_blocks() == 64
    finally:
        eng.close()


def test_engine_publishes_nothing_after_a_failed_prefill(llm, monkeypatch):
    eng, kv = _engine(llm, prefill_chunk=64)
    real = llm.prefill

    def failing(x, kv=None, slots=None, start_pos=0, prefix_blocks=None):
        if start_pos >= 128:
            raise RuntimeError("boom")
        return real(x, kv, slots, start_pos=start_pos, prefix_blocks=prefix_blocks)

    try:
        p = _prompts()[0]
        monkeypatch.setattr(llm, "prefill", failing)
        r = eng.submit(p, len(p), SamplingParams(max_new_tokens=4), prefix_keys=_pk(p))
        with pytest.raises(RuntimeError, match="boom"):
            list(r.stream(timeout=120))
        assert kv.blocks.cached_blocks() == 0 and kv.blocks.num_seqs() == 0 and kv.blocks.free_blocks() == 64
        assert kv.blocks.match(_pk(p), 1 << 40) == 0
        monkeypatch.setattr(llm, "prefill", real)
        ok = _run(eng, [p], keys=True)[0]
        assert ok.cached_tokens == 0 and kv.blocks.cached_blocks() == 2
    finally:
        eng.close()


# ----------------------------------------------------------------------------- key builder
def _match_tokens(published, probe):
    bm = BlockManager(16)
    assert bm.reserve(1, len(published) * 64)
    bm.publish(1, published)
    return bm.match(probe, 2)


def test_key_builder():
    rng = np.random.default_rng(0)
    IMG = 259
    text_a = [int(t) for t in rng.integers(0, 250, 70)]
    tail = [int(t) for t in rng.integers(0, 250, 150)]
    ids = text_a + [IMG] * 100 + tail                      # image rows 70 .. 169: blocks 1 and 2
    d1, d2 = b"\x01" * 16, b"\x02" * 16
    base = prefix_cache_keys(ids, [70], d1)
    assert base.shape == (5, 2) and base.dtype == np.uint64
    assert np.array_equal(base, prefix_cache_keys(ids, [70], d1))
    # same text, different image: the match stops before the first block with an image row
    assert _match_tokens(base, prefix_cache_keys(ids, [70], d2)) == 64
    # same image, different question: the match covers the image span
    other = ids[:200] + [int(t) for t in rng.integers(0, 250, 130)]
    assert _match_tokens(base, prefix_cache_keys(other, [70], d1)) == 192 >= 170
    # one token changed inside block j: the match ends at j
    for j in range(5):
        ch = list(ids)
        ch[64 * j + 9] = 251
        assert _match_tokens(base, prefix_cache_keys(ch, [70], d1)) == 64 * j
    # no image: the digest plays no part
    assert np.array_equal(prefix_cache_keys(tail, [], d1), prefix_cache_keys(tail, [], d2))


# ----------------------------------------------------------------------------- service
def _service(tmp_path, monkeypatch, enabled):
    from lumen_amd.models.vlm import write_vlm_model
    from lumen_amd.resources.validator import config_from_dict
    from lumen_amd.services.vlm import GeneralFastVLMService

    if enabled:
        monkeypatch.setenv("LUMEN_PREFIX_CACHE", "1")
    else:
        monkeypatch.delenv("LUMEN_PREFIX_CACHE", raising=False)
    write_vlm_model(tmp_path / "models" / "fastvlm-tiny", "fastvlm-tiny")
    cfg = {"metadata": {"version": "1.0.0", "region": "other", "cache_dir": str(tmp_path)},
           "deployment": {"mode": "single", "service": "vlm"}, "server": {"port": 50557, "host": "127.0.0.1"},
           "services": {"vlm": {"enabled": True, "package": "lumen_vlm",
                                "import_info": {"registry_class": "lumen_vlm.fastvlm.GeneralFastVLMService",
                                                "add_to_server": "lumen_vlm.proto.ml_service_pb2_grpc.add_InferenceServicer_to_server"},
                                "backend_settings": {"device": "cpu"},
                                "models": {"general": {"model": "fastvlm-tiny", "runtime": "onnx"}}}}}
    s = GeneralFastVLMService.from_config(config_from_dict(cfg).services["vlm"], tmp_path)
    s.initialize()
    calls = []
    real = s.backend.model.encode_images

    def spy(images, out=None):
        calls.append(len(images))
        return real(images, out=out)

    s.backend.model.encode_images = spy
    return s, calls


def _img():
    from lumen_amd.utils.image import encode_jpeg

    return encode_jpeg(np.random.default_rng(0).integers(0, 255, (40, 60, 3), dtype=np.uint8))


_LONG = "Look at the picture carefully and answer in one short sentence, naming colours and shapes. "


@pytest.mark.parametrize("enabled", [True, False])
def test_service_second_request_reuses_the_image(tmp_path, monkeypatch, enabled):
    from lumen_amd.proto import ml_service as pb

    s, calls = _service(tmp_path, monkeypatch, enabled)
    try:
        img = _img()
        body1, _, m1 = s.handle("vlm_generate", img, "image/jpeg", {"prompt": _LONG + "What is it?", "max_new_tokens": "5"})
        assert json.loads(body1)["input_tokens"] > 80 and m1["cached_tokens"] == "0" and calls == [1]
        body2, _, m2 = s.handle("vlm_generate", img, "image/jpeg", {"prompt": _LONG + "Where is it?", "max_new_tokens": "5"})
        req = pb.InferRequest(correlation_id="s1", task="vlm_generate_stream", payload=img, payload_mime="image/jpeg",
                              meta={"prompt": _LONG + "Why?", "max_new_tokens": "4"})
        out = list(s.Infer(iter([req]), None))
        assert out[-1].is_final
        if enabled:
            assert int(m2["cached_tokens"]) >= 64 and int(out[-1].meta["cached_tokens"]) >= 64
            assert calls == [1], "the vision tower ran again on a prefix hit"
            assert "t_decode_ms" not in out[-1].meta and "t_prefix_ms" in out[-1].meta   # no JPEG decode either
            # the same request again generates what the cold engine generated
            body3, _, m3 = s.handle("vlm_generate", img, "image/jpeg",
                                    {"prompt": _LONG + "What is it?", "max_new_tokens": "5"})
            assert int(m3["cached_tokens"]) >= 64 and json.loads(body3)["text"] == json.loads(body1)["text"]
            # another image under the same text: its rows are not shared
            from lumen_amd.utils.image import encode_jpeg

            other = encode_jpeg(np.random.default_rng(1).integers(0, 255, (40, 60, 3), dtype=np.uint8))
            _, _, m4 = s.handle("vlm_generate", other, "image/jpeg", {"prompt": _LONG + "What is it?", "max_new_tokens": "5"})
            assert m4["cached_tokens"] == "0" and calls == [1, 1]
        else:
            assert m2["cached_tokens"] == "0" and out[-1].meta["cached_tokens"] == "0"
            assert calls == [1, 1, 1] and "t_decode_ms" in out[-1].meta
            assert s.backend.kv.blocks.cached_blocks() == 0
    finally:
        s.close()
