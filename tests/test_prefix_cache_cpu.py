"""Prefix caching across generate() calls on the CPU: PagedKVCache.truncate
and LlamaBackend(prefix_cache=...) on tiny-debug
(tests/prefix_cache_cases.py)."""

import pytest
import torch

import prefix_cache_cases as cc
from senweaver_amd.engine.kvcache import PagedKVCache
from senweaver_amd.models.config import get_config

DEV = "cpu"


# ---------------- PagedKVCache.truncate ----------------
def _cache(num_pages=8):
    return PagedKVCache(get_config("tiny-debug"), num_pages, torch.device("cpu"))


def _balanced(cache):
    owned = [p for bt in cache.block_tables for p in bt]
    assert len(cache._free) + len(owned) == cache.num_pages
    assert len(set(cache._free) | set(owned)) == cache.num_pages


@pytest.mark.parametrize("length,new_len,pages_left", [
    (50, 50, 4), (50, 49, 4), (50, 48, 3), (50, 33, 3), (50, 32, 2),
    (50, 17, 2), (50, 16, 1), (50, 1, 1), (50, 0, 0), (64, 64, 4), (64, 63, 4)])
def test_truncate_returns_whole_pages(length, new_len, pages_left):
    cache = _cache()
    other = cache.new_seq()
    cache._ensure_capacity(other, 20)
    cache.seq_lens[other] = 20
    seq = cache.new_seq()
    cache._ensure_capacity(seq, length)
    cache.seq_lens[seq] = length
    kept = list(cache.block_tables[seq][:pages_left])
    dropped = cache.block_tables[seq][pages_left:]
    _balanced(cache)
    cache.truncate(seq, new_len)
    assert cache.seq_lens[seq] == new_len
    assert cache.block_tables[seq] == kept
    assert all(p in cache._free for p in dropped)
    assert cache.seq_lens[other] == 20 and len(cache.block_tables[other]) == 2
    _balanced(cache)
    cache._ensure_capacity(seq, length)      # grows again from the free list
    _balanced(cache)


def test_truncate_rejects_growth_and_negative():
    cache = _cache()
    seq = cache.new_seq()
    cache._ensure_capacity(seq, 20)
    cache.seq_lens[seq] = 20
    for bad in (21, -1):
        with pytest.raises(ValueError):
            cache.truncate(seq, bad)
    assert cache.seq_lens[seq] == 20
    _balanced(cache)


def test_truncate_recovers_pages_of_an_unfinished_append():
    """Pages taken for positions the logical length never reached."""
    cache = _cache()
    seq = cache.new_seq()
    cache._ensure_capacity(seq, 40)
    cache.seq_lens[seq] = 10
    cache.truncate(seq, 10)
    assert len(cache.block_tables[seq]) == 1
    _balanced(cache)


# ---------------- LlamaBackend(prefix_cache=...) ----------------
@pytest.fixture(scope="module")
def two_turns():
    with torch.no_grad():
        return cc.check_two_turns(DEV)


def test_second_turn_extends_once(two_turns):
    on, spy, _, _ = two_turns
    assert on.prefix_cache and len(spy.extend) >= 1


def test_default_is_off_and_env_turns_it_on(monkeypatch):
    monkeypatch.delenv("SENWEAVER_PREFIX_CACHE", raising=False)
    b = cc.LlamaBackend("tiny-debug", device=DEV, seed=0, max_seq=cc.MAX_SEQ)
    assert b.prefix_cache is False
    spy = cc.Spy(b)
    r1, _ = cc.generate(b, cc.TURN1)
    cc.generate(b, cc.next_turn(cc.TURN1, r1, 0))
    assert not spy.extend and len(spy.prefill) == 2
    assert b._cached_ids is None
    assert b.prefix_cache_stats()["hits"] == 0
    monkeypatch.setenv("SENWEAVER_PREFIX_CACHE", "1")
    assert cc.LlamaBackend("tiny-debug", device=DEV, max_seq=64).prefix_cache is True
    monkeypatch.setenv("SENWEAVER_PREFIX_CACHE", "0")
    assert cc.LlamaBackend("tiny-debug", device=DEV, max_seq=64).prefix_cache is False
    assert cc.LlamaBackend("tiny-debug", device=DEV, max_seq=64,
                           prefix_cache=True).prefix_cache is True


def test_identical_prompt_reuse_is_capped():
    on, off = cc.make_backend(DEV, True), cc.make_backend(DEV, False)
    spy = cc.Spy(on)
    a, _ = cc.generate(on, cc.TURN1)
    b, _ = cc.generate(on, cc.TURN1)
    ids = cc.prompt_ids(on, cc.render(cc.TURN1))
    assert spy.extend[0]["new_lens"] == [1]
    assert spy.extend[0]["tokens"][0, 0] == ids[-1]
    assert on.prefix_cache_stats()["tokens_reused"] == len(ids) - 1
    ref, _ = cc.generate(off, cc.TURN1)
    assert a == ref and b == ref


def test_unrelated_prompt_matches_off():
    """Only BOS is shared: output and page accounting as with the cache off."""
    on, off = cc.make_backend(DEV, True), cc.make_backend(DEV, False)
    cc.generate(on, cc.TURN1)
    cc.generate(off, cc.TURN1)
    got, _ = cc.generate(on, cc.UNRELATED)
    ref, _ = cc.generate(off, cc.UNRELATED)
    assert got == ref
    c_on, c_off = on._decode_cache, off._decode_cache
    assert c_on.seq_lens == c_off.seq_lens
    assert len(c_on.block_tables[0]) == len(c_off.block_tables[0])
    assert len(c_on._free) == len(c_off._free)
    assert on.prefix_cache_stats()["tokens_reused"] == 1     # BOS


def test_aborted_turn_keeps_a_true_record_and_next_turn_reuses():
    on = cc.make_backend(DEV, True)
    spy = cc.Spy(on)
    chunks = []
    text = on.stream_generate(cc.render(cc.TURN1), cc.MAX_NEW,
                              lambda: len(chunks) >= 2, chunks.append)
    cc.assert_pages(on)
    assert len(chunks) == 2
    ids1 = cc.prompt_ids(on, cc.render(cc.TURN1))
    n = on._decode_cache.seq_lens[0]
    assert n == len(ids1) + 2
    assert len(on._cached_ids) == n and on._cached_ids[:len(ids1)] == ids1
    assert on.tokenizer.decode(on._cached_ids[len(ids1):]) == text
    cc.generate(on, cc.next_turn(cc.TURN1, text, 0))
    assert len(spy.extend) == 1 and len(spy.prefill) == 1
    assert on.prefix_cache_stats()["hits"] == 1


def test_exception_in_prefill_clears_the_record():
    on = cc.make_backend(DEV, True)
    r1, _ = cc.generate(on, cc.TURN1)
    inner = on.model.prefill_extend

    def boom(*a, **k):
        raise RuntimeError("boom")

    on.model.prefill_extend = boom
    with pytest.raises(RuntimeError):
        cc.generate(on, cc.next_turn(cc.TURN1, r1, 0))
    assert on._cached_ids is None
    on.model.prefill_extend = inner
    spy = cc.Spy(on)
    cc.generate(on, cc.next_turn(cc.TURN1, r1, 0))     # full reset, no reuse
    assert len(spy.prefill) == 1 and not spy.extend


def test_three_turns_keep_accounts(two_turns):
    on, spy, turn2, r2 = two_turns
    before = len(spy.extend)
    cc.generate(on, cc.next_turn(turn2, r2, 1))
    assert len(spy.extend) == before + 1 and len(spy.prefill) == 1
    st = on.prefix_cache_stats()
    assert st["calls"] == 3 and st["hits"] == 2


def test_http_server_flag():
    import inspect

    from senweaver_amd.server import http_api
    assert "--prefix-cache" in inspect.getsource(http_api)
