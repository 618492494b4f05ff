"""Prefix caching: time to first token of turn 2, cache on against off.

Llama-3-8B bf16 on one GPU, max_seq 2048.  A synthetic two-turn exchange is
built from seeded token ids (the tokenizer is not involved, so the lengths
are exact): turn 1 leaves ``history`` tokens in the KV cache, turn 2's
prompt is those tokens plus ``suffix`` new ones.  Timed, per repetition:
the prompt phase of ``LlamaBackend.stream_generate`` on turn 2's ids
(``_prefill_prompt``: common-prefix search, truncate and prefill_extend of
the suffix when the cache is on; the full reset and prefill of every token
when it is off, which is the code path from before prefix caching), the
lm_head on the last position and the greedy pick, ending in a device
synchronise.  Untimed, before every repetition of either kind: turn 1's
prefill, so both start from the same device state.

On and off alternate in one process, on one backend (the switch is the
``prefix_cache`` attribute), after warm-up of every shape involved.

    python benchmarks/prefix_cache_bench.py [--reps 7] [--out PATH]
    python benchmarks/prefix_cache_bench.py --profile   # one pass, for rocprofv3

The attention cost model (FLOPs and bytes of paged_prefill_attn from shapes)
is printed with the results and used by profiles/prefix_cache_breakdown.txt.
"""

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from senweaver_amd import ops  # noqa: E402
from senweaver_amd.engine.scorer import LlamaBackend  # noqa: E402

MAX_SEQ = 2048
CONFIGS = [(1920, 128), (2040, 8)]   # (history, suffix)
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                           "results", "prefix_cache_llama8b.json")


def attn_cost(history, suffix, H, Hk, D=128, qblk=64, kvblk=64):
    """paged_prefill_attn, one layer, B = 1, from shapes alone.

    flops_needed: 2 matmuls x 2 D per (row, visible key).  flops_issued: what
    the 64 x 64 tiles execute (whole tiles, pad rows included).  bytes_min:
    Q and O once, K and V of the context once per kv head.  bytes_read: as
    the kernel reads them, K and V tiles once per (query block, query head).
    """
    ctx = history + suffix
    Sq = (suffix + 63) // 64 * 64
    visible = sum(history + i + 1 for i in range(suffix))
    tiles = 0
    for qb in range((Sq + qblk - 1) // qblk):
        if qb * qblk >= suffix:
            continue
        kv_end = history + min(suffix, qb * qblk + qblk)
        tiles += (kv_end + kvblk - 1) // kvblk
    qo = 2 * suffix * H * D * 2
    return dict(
        flops_needed=4 * D * H * visible,
        flops_issued=4 * D * H * tiles * qblk * kvblk,
        bytes_min=qo + 2 * ctx * Hk * D * 2,
        bytes_read=qo + H * tiles * kvblk * D * 2 * 2,
    )


def turn_ids(vocab, history, suffix, seed=5):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab, (history + suffix,), generator=g).tolist()
    return ids[:history], ids


def first_token(backend, cache, ids):
    last = backend._prefill_prompt(cache, ids)
    tok_id = int(ops.argmax_rows(backend.model.logits(last.reshape(1, -1)))[0])
    torch.cuda.synchronize()
    return tok_id


def turn2_ms(backend, cache, hist_ids, ids, on):
    """One repetition: untimed turn 1, timed turn 2."""
    backend.prefix_cache = on
    backend._cached_ids = None
    backend._prefill_prompt(cache, hist_ids)          # full reset + prefill
    backend._cached_ids = list(hist_ids) if on else None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tok_id = first_token(backend, cache, ids)
    return (time.perf_counter() - t0) * 1e3, tok_id


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--profile", action="store_true",
                    help="warm up, then one on and one off pass per config; "
                         "no timing, no file (run under rocprofv3)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prefix_cache_bench needs a GPU: a CPU timing says nothing")
    if args.reps < 5 and not args.profile:
        raise SystemExit("--reps must be at least 5")

    with torch.no_grad():
        backend = LlamaBackend("llama-3-8b", max_seq=MAX_SEQ, prefix_cache=True)
        cfg = backend.config
        cache, _ = backend._decode_state()
        results = []
        for history, suffix in CONFIGS:
            hist_ids, ids = turn_ids(cfg.vocab_size, history, suffix)
            for _ in range(args.warmup):
                for on in (True, False):
                    turn2_ms(backend, cache, hist_ids, ids, on)
            n = 1 if args.profile else args.reps
            on_ms, off_ms, toks = [], [], set()
            hits0 = backend.prefix_cache_stats()["hits"]
            for _ in range(n):
                for on, sink in ((True, on_ms), (False, off_ms)):
                    ms, tok_id = turn2_ms(backend, cache, hist_ids, ids, on)
                    sink.append(ms)
                    toks.add((on, tok_id))
            assert backend.prefix_cache_stats()["hits"] - hits0 == n, "cache not hit"
            cost = attn_cost(history, suffix, cfg.num_heads, cfg.num_kv_heads)
            r = dict(history=history, suffix=suffix,
                     on_ms=[round(x, 3) for x in on_ms],
                     off_ms=[round(x, 3) for x in off_ms],
                     on_median_ms=round(statistics.median(on_ms), 3),
                     off_median_ms=round(statistics.median(off_ms), 3),
                     on_spread_ms=round(max(on_ms) - min(on_ms), 3),
                     off_spread_ms=round(max(off_ms) - min(off_ms), 3),
                     speedup_of_medians=round(statistics.median(off_ms)
                                              / statistics.median(on_ms), 3),
                     same_first_token=len({t for _, t in toks}) == 1,
                     attn_cost_per_layer=cost)
            results.append(r)
            print(json.dumps(r))
    if args.profile:
        return
    doc = dict(benchmark="prefix_cache_bench", model="llama-3-8b", quant="bf16",
               gpus=1, max_seq=MAX_SEQ, reps=args.reps, warmup=args.warmup,
               metric="time to first token of turn 2, ms (prompt phase + lm_head "
                      "+ argmax, device synchronised; profiler off)",
               device=torch.cuda.get_device_name(0), results=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
