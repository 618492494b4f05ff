"""Prefix caching across generate() calls on the GPU, with the captured
decode graph (tests/prefix_cache_cases.py)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import prefix_cache_cases as cc
from senweaver_amd import ops
from senweaver_amd.engine import tokenizer as tok
from senweaver_amd.engine.kvcache import PagedKVCache

DEV = "cuda:0"


@pytest.fixture(scope="module")
def two_turns():
    assert torch.cuda.is_available()
    assert ops.extension_loaded(), "HIP extension failed to build/load"
    with torch.no_grad():
        return cc.check_two_turns(DEV)


def test_second_turn_extends_once_gpu(two_turns):
    on, spy, _, _ = two_turns
    assert on._decode_graph is not None and len(spy.extend) >= 1


def test_identical_and_unrelated_prompts_gpu(two_turns):
    on, off = cc.make_backend(DEV, True), cc.make_backend(DEV, False)
    spy = cc.Spy(on)
    a, _ = cc.generate(on, cc.TURN1)
    ref, _ = cc.generate(off, cc.TURN1)
    assert a == ref
    cc.generate(on, cc.TURN1)
    ids = cc.prompt_ids(on, cc.render(cc.TURN1))
    assert spy.extend[0]["new_lens"] == [1]
    assert on.prefix_cache_stats()["tokens_reused"] == len(ids) - 1
    got, _ = cc.generate(on, cc.UNRELATED)
    exp, _ = cc.generate(off, cc.UNRELATED)
    assert got == exp
    assert on._decode_cache.seq_lens == off._decode_cache.seq_lens
    assert len(on._decode_cache._free) == len(off._decode_cache._free)


def test_aborted_turn_then_reuse_gpu(two_turns):
    on = cc.make_backend(DEV, True)
    spy = cc.Spy(on)
    chunks = []
    text = on.stream_generate(cc.render(cc.TURN1), cc.MAX_NEW,
                              lambda: len(chunks) >= 2, chunks.append)
    cc.assert_pages(on)
    ids1 = cc.prompt_ids(on, cc.render(cc.TURN1))
    n = on._decode_cache.seq_lens[0]
    assert n == len(ids1) + 2 and len(on._cached_ids) == n
    assert on._cached_ids[:len(ids1)] == ids1
    cc.generate(on, cc.next_turn(cc.TURN1, text, 0))
    assert len(spy.extend) == 1 and on.prefix_cache_stats()["hits"] == 1


@torch.no_grad()
def test_third_turn_decodes_through_the_graph(two_turns):
    """4 tokens after an extend through DecodeGraph == the same steps with
    model.decode_step, eagerly, from a copy of the cache state."""
    on, spy, turn2, r2 = two_turns
    model, cache = on.model, on._decode_cache
    snap = {}
    inner = model.prefill_extend          # the spy's wrapper

    def extend_and_snapshot(tokens, cache_, seqs, new_lens):
        out = inner(tokens, cache_, seqs, new_lens)
        copy = PagedKVCache(model.config, cache_.num_pages, model.device,
                            num_kv_heads=model.local_kv_heads)
        for dst, src in zip(copy.k + copy.v, cache_.k + cache_.v):
            dst.copy_(src)
        copy.block_tables = [list(bt) for bt in cache_.block_tables]
        copy.seq_lens = list(cache_.seq_lens)
        owned = {p for bt in copy.block_tables for p in bt}
        copy._free = [p for p in copy._free if p not in owned]
        snap["cache"], snap["last"] = copy, out[0, new_lens[0] - 1].clone()
        return out

    fed = []
    inner_decode = on._decode_one
    on._decode_one = lambda c, g, s, t: (fed.append(t), inner_decode(c, g, s, t))[1]
    model.prefill_extend = extend_and_snapshot
    try:
        cc.generate(on, cc.next_turn(turn2, r2, 1), max_new=4)
    finally:
        model.prefill_extend = inner
        on._decode_one = inner_decode
    assert on._decode_graph.graph is not None, "decode must go through the graph"
    assert "cache" in snap, "turn 3 must extend"

    eager, h, c2 = [], snap["last"], snap["cache"]
    for _ in range(4):
        nxt = int(ops.argmax_rows(model.logits(h.reshape(1, -1)))[0])
        if nxt == tok.EOS:
            break
        eager.append(nxt)
        pos = torch.tensor([c2.seq_lens[0]], device=model.device)
        h = model.decode_step(torch.tensor([nxt], device=model.device), pos, c2, [0])[0]
    assert fed == eager
    assert len(fed) == 4 or len(fed) == len(eager)
