"""Shared pieces of the prefix-cache tests (CPU and GPU); no tests here.

A conversation is rendered with LLMMessageService.render_messages, exactly
as the agent loop and the servers do; turn k+1 is turn k plus the reply and
a new user message.  ``Spy`` wraps a backend's model so that every call of
``prefill`` and ``prefill_extend`` is recorded (and still runs).
"""

import torch

import prefix_pack_cases as pc
from senweaver_amd.engine import tokenizer as tok
from senweaver_amd.engine.scorer import LlamaBackend
from senweaver_amd.transport.service import LLMChatMessage, LLMMessageService

MAX_SEQ = 512
MAX_NEW = 8

TURN1 = [
    LLMChatMessage("system", "You are a careful coding agent. Use tools when needed."),
    LLMChatMessage("user", "List the files in src/ and tell me which one defines the parser."),
]
FOLLOW_UPS = ["Now open it and show me the first function.",
              "Rename that function to parse_document and run the tests."]
# a raw prompt (not rendered): its first token differs from "<|system|>"'s
UNRELATED = "What is the capital of France?"


def make_backend(device, prefix_cache):
    return LlamaBackend("tiny-debug", device=device, seed=0, max_seq=MAX_SEQ,
                        prefix_cache=prefix_cache)


def render(messages):
    return LLMMessageService.render_messages(messages)


def next_turn(messages, reply, k):
    return messages + [LLMChatMessage("assistant", reply),
                       LLMChatMessage("user", FOLLOW_UPS[k])]


def prompt_ids(backend, prompt, max_new=MAX_NEW):
    """The ids stream_generate builds for this prompt."""
    budget = backend.max_seq - max_new - 8
    return ([tok.BOS] + backend.tokenizer.encode(prompt, max_tokens=budget)
            + [tok.ROLE_ASSISTANT])


def lcp(a, b):
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


class Spy:
    def __init__(self, backend):
        self.prefill, self.extend = [], []
        model = backend.model
        inner_p, inner_e = model.prefill, model.prefill_extend

        def prefill(tokens, cache=None, seqs=None, real_lens=None):
            self.prefill.append(real_lens)
            return inner_p(tokens, cache=cache, seqs=seqs, real_lens=real_lens)

        def prefill_extend(tokens, cache, seqs, new_lens):
            out = inner_e(tokens, cache, seqs, new_lens)
            self.extend.append(dict(tokens=tokens.cpu(), new_lens=list(new_lens),
                                    last=out[0, new_lens[0] - 1].clone()))
            return out

        model.prefill, model.prefill_extend = prefill, prefill_extend


def assert_pages(backend):
    """free + owned == num_pages, no page twice, enough pages for the length."""
    cache = backend._decode_cache
    owned = [p for bt in cache.block_tables for p in bt]
    assert len(cache._free) + len(owned) == cache.num_pages
    assert len(set(cache._free) | set(owned)) == cache.num_pages
    for bt, n in zip(cache.block_tables, cache.seq_lens):
        assert len(bt) * 16 >= n


def generate(backend, messages, max_new=MAX_NEW, should_stop=None):
    """(text, cumulative chunks) of one greedy turn; page accounting checked."""
    chunks = []
    prompt = messages if isinstance(messages, str) else render(messages)
    text = backend.stream_generate(prompt, max_new,
                                   should_stop or (lambda: False), chunks.append)
    assert_pages(backend)
    return text, chunks


def decode_path_last_hidden(model, ids, m):
    """Noise pair, on code that predates the prefix cache: (prefill of ids,
    last row) against (prefill of ids[:m], then decode_step token by token,
    last row).  Returns (decode_last, prefill_last)."""
    from senweaver_amd.engine.kvcache import PagedKVCache
    dev = model.device

    def pad(x):
        S = (len(x) + 127) & ~127
        t = torch.zeros(1, S, dtype=torch.long)
        t[0, :len(x)] = torch.tensor(x)
        return t.to(dev)

    full = model.prefill(pad(ids))[0, len(ids) - 1]
    cache = PagedKVCache(model.config, MAX_SEQ // 16 + 2, dev,
                         num_kv_heads=model.local_kv_heads)
    seq = cache.new_seq()
    model.prefill(pad(ids[:m]), cache=cache, seqs=[seq], real_lens=[m])
    h = None
    for p in range(m, len(ids)):
        h = model.decode_step(torch.tensor([ids[p]], device=dev),
                              torch.tensor([p], device=dev), cache, [seq])[0]
    return h, full


def check_two_turns(device):
    """Turn 2 with the cache on: one prefill_extend of len(ids) - lcp tokens,
    no prefill, stats agree, last-position hidden within 2x the decode-path
    noise of the full prefill.  Returns (on backend, spy, turn-2 messages,
    turn-2 reply)."""
    on, off = make_backend(device, True), make_backend(device, False)
    spy, spy_off = Spy(on), Spy(off)
    r1, _ = generate(on, TURN1)
    r1_off, _ = generate(off, TURN1)
    assert r1 == r1_off, "turn 1 takes the same path on and off"
    ids1 = prompt_ids(on, render(TURN1))
    assert spy.prefill == [[len(ids1)]] and not spy.extend
    cached = list(on._cached_ids)
    assert cached[:len(ids1)] == ids1
    assert len(cached) == on._decode_cache.seq_lens[0]

    turn2 = next_turn(TURN1, r1, 0)
    ids2 = prompt_ids(on, render(turn2))
    m = lcp(cached, ids2)
    assert 16 < m < len(ids2) - 1, "the conversation must share a real prefix"
    r2, _ = generate(on, turn2)
    assert len(spy.prefill) == 1, "model.prefill must not run on turn 2"
    assert len(spy.extend) == 1
    e = spy.extend[0]
    n = len(ids2) - m
    assert e["new_lens"] == [n]
    assert e["tokens"].shape[1] % 64 == 0 and e["tokens"].shape[1] - n < 64
    assert e["tokens"][0, :n].tolist() == ids2[m:]
    assert on.prefix_cache_stats() == dict(
        calls=2, hits=1, tokens_reused=m, tokens_prefilled=len(ids1) + n)

    generate(off, turn2)
    assert not spy_off.extend and len(spy_off.prefill) == 2
    assert off.prefix_cache_stats()["hits"] == 0

    dec_last, full_last = decode_path_last_hidden(off.model, ids2, m)
    pc.assert_within_noise(f"prefix cache turn 2 ({device}) last hidden",
                           e["last"], full_last, dec_last, full_last)
    return on, spy, turn2, r2
