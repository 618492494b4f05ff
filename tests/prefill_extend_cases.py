"""Shared pieces of the prefill_extend tests (CPU and GPU); no tests here.

One seeded 192-token row on tiny-debug.  ``prefill`` of all 192 tokens is
the reference.  The tolerance is MEASURED on code that predates
prefill_extend: the history is prefilled into a cache and the following
tokens go through ``decode_step`` one at a time; those hidden rows differ
from the reference rows by another attention kernel and another GEMM row
count.  ``prefill_extend`` differs from the full prefill by the same kinds
of change, in two places at once (as in prefix_pack_cases), hence within 2x
that noise, in max abs and in max relative difference.  The same rule
judges the K/V the extend wrote into the cache (reference: the K/V a full
prefill writes at those positions; noise: the decode loop's against them).
"""

import torch

import kernel_oracles as ko
import prefix_pack_cases as pc

TOTAL = 192
NUM_PAGES = 16


def token_row(vocab, seed=11, lo=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, vocab, (1, TOTAL), generator=g)


def sentinel_cache(model):
    from senweaver_amd.engine.kvcache import PagedKVCache
    cache = PagedKVCache(model.config, NUM_PAGES, model.device,
                         num_kv_heads=model.local_kv_heads)
    for t in cache.k + cache.v:
        t.fill_(ko.SENTINEL)
    return cache


def _pad64(row, n):
    S = (n + 63) & ~63
    out = torch.zeros(1, S, dtype=torch.long)
    out[0, :n] = row[0, :n]
    return out


def prefill_history(model, row, hist):
    cache = sentinel_cache(model)
    seq = cache.new_seq()
    model.prefill(_pad64(row, hist).to(model.device), cache=cache, seqs=[seq],
                  real_lens=[hist])
    assert cache.seq_lens[seq] == hist
    return cache, seq


def kv_rows(cache, seq, start, count):
    """K and V of positions [start, start+count) of every layer:
    ([L, count, Hk, D], same) on the CPU."""
    sl = cache.slot_ids(seq, start, count)
    P = cache.num_pages
    k = torch.stack([t.view(P * 16, *t.shape[2:])[sl] for t in cache.k]).cpu()
    v = torch.stack([t.view(P * 16, *t.shape[2:])[sl] for t in cache.v]).cpu()
    return k, v


class Reference:
    """Full prefill of the 192 tokens: hidden rows and cache K/V, once."""

    def __init__(self, model):
        self.row = token_row(model.config.vocab_size)
        self.cache = sentinel_cache(model)
        self.seq = self.cache.new_seq()
        self.hidden = model.prefill(self.row.to(model.device), cache=self.cache,
                                    seqs=[self.seq], real_lens=[TOTAL])[0].cpu()


def check_extend(model, ref, hist, n, Sq):
    """prefill(hist) + prefill_extend(n tokens padded to Sq) against ref."""
    assert hist + n <= TOTAL and n <= Sq
    row, dev = ref.row, model.device
    ref_h = ref.hidden[hist:hist + n]
    ref_k, ref_v = kv_rows(ref.cache, ref.seq, hist, n)

    # noise pair: today's decode path, token by token
    cache_d, seq_d = prefill_history(model, row, hist)
    dec = []
    for p in range(hist, hist + n):
        dec.append(model.decode_step(row[0, p:p + 1].to(dev),
                                     torch.tensor([p], device=dev), cache_d, [seq_d])[0])
    dec_h = torch.stack(dec).cpu()
    dec_k, dec_v = kv_rows(cache_d, seq_d, hist, n)

    # under test
    cache_e, seq_e = prefill_history(model, row, hist)
    before_k = [t.clone() for t in cache_e.k]
    before_v = [t.clone() for t in cache_e.v]
    tokens = torch.zeros(1, Sq, dtype=torch.long)
    tokens[0, :n] = row[0, hist:hist + n]
    out = model.prefill_extend(tokens.to(dev), cache_e, [seq_e], [n])
    assert tuple(out.shape) == (1, Sq, model.config.hidden_size)
    assert cache_e.seq_lens[seq_e] == hist + n, "seq_lens must advance once, by n"
    assert len(cache_e._free) + len(cache_e.block_tables[seq_e]) == NUM_PAGES

    what = f"prefill_extend {dev.type} hist={hist} n={n} Sq={Sq}"
    pc.assert_within_noise(what + " hidden", out[0, :n].cpu(), ref_h, dec_h, ref_h)
    ext_k, ext_v = kv_rows(cache_e, seq_e, hist, n)
    pc.assert_within_noise(what + " cache K", ext_k, ref_k, dec_k, ref_k)
    pc.assert_within_noise(what + " cache V", ext_v, ref_v, dec_v, ref_v)

    # everything but the n new slots is bit-unchanged: history, the rest of
    # the last page, pages the sequence does not own (sentinel)
    P = cache_e.num_pages
    keep = torch.ones(P * 16, dtype=torch.bool)
    keep[cache_e.slot_ids(seq_e, hist, n).cpu()] = False
    for name, now, was in (("K", cache_e.k, before_k), ("V", cache_e.v, before_v)):
        for li in range(len(now)):
            a = now[li].view(P * 16, -1).cpu()[keep]
            b = was[li].view(P * 16, -1).cpu()[keep]
            ko.assert_bits_equal(a, b, f"{what}: stray {name}-cache write, layer {li}")
    owned = set(cache_e.block_tables[seq_e])
    for pg in range(P):
        if pg not in owned:
            assert bool((cache_e.k[0][pg] == ko.SENTINEL).all())
