"""Input builders and check drivers for paged_prefill_attn, shared by
test_paged_prefill_gpu.py (the HIP kernel) and test_paged_prefill_cpu.py
(the fp32 reference behind ops.paged_prefill_attn).  No tests live here.

The op under test is
``fn(q [B,Sq,H,D], kcache, vcache, block_table, ctx_lens, q_lens, scale)
-> o [B,Sq,H,D]``: query row i of sequence b sits at position
ctx - q_len + i and sees keys 0 .. that position of the paged cache.

A paged case is made from a contiguous one (kernel_oracles' pointer, decoy
and random generators, K/V [B,Hk,S,D] with S = ctx): K/V are scattered into
a page pool through a random page permutation, unused block-table entries
are -1, the table has spare columns and the pool spare pages, and every
slot that no position maps to holds random finite data.  The queries are
the last q_len rows of the contiguous Q.
"""

from __future__ import annotations

import math

import torch

import kernel_oracles as ko

BF16 = torch.bfloat16
PAGE = ko.PAGE
BF16_MAX = float(torch.finfo(BF16).max)

# (ctx, q_len): no history; history on a tile edge; decode-shaped;
# verify-shaped with history % 16 == 1; one row past a wave; one row past a
# block with the history straddling a KV tile; several blocks and tiles
CASES = [(64, 64), (80, 16), (100, 1), (150, 5), (200, 17), (333, 65), (700, 200)]
HEAD_CONFIGS = [(1, 1, 1), (2, 4, 2), (1, 6, 2)]   # (B, H, Hk); ratio 3 last
# B = 2 with different geometry per sequence; every case appears
RANDOM_PAIRS = [((64, 64), (80, 16)), ((100, 1), (150, 5)),
                ((200, 17), (333, 65)), ((700, 200), (150, 5))]


def scatter_paged(gen, k, v, spare_pages=5, spare_cols=3):
    """k, v [B,Hk,S,D] -> (kcache, vcache [P,16,Hk,D], block_table [B,maxp]
    int32, slots [B,S] int64).  Pool pre-filled with random data."""
    B, Hk, S, D = k.shape
    need = -(-S // PAGE)
    P = B * need + spare_pages
    perm = torch.randperm(P, generator=gen)
    bt = torch.full((B, need + spare_cols), -1, dtype=torch.int32)
    kc = ko.rand_bf16(gen, P, PAGE, Hk, D)
    vc = ko.rand_bf16(gen, P, PAGE, Hk, D)
    kflat, vflat = kc.view(P * PAGE, Hk, D), vc.view(P * PAGE, Hk, D)
    slots = []
    for b in range(B):
        bt[b, :need] = perm[b * need:(b + 1) * need].to(torch.int32)
        sl = ko.slots_of(bt[b], S)
        kflat[sl] = k[b].transpose(0, 1)
        vflat[sl] = v[b].transpose(0, 1)
        slots.append(sl)
    return kc, vc, bt, torch.stack(slots)


def tail_rows(x, q_len):
    """[B,H,S,D] -> its last q_len rows, token-major [B,q_len,H,D]."""
    return x[:, :, x.shape[2] - q_len:].permute(0, 2, 1, 3).contiguous()


def call(fn, dev, q, kc, vc, bt, ctxs, qlens, scale):
    t = lambda xs: torch.tensor(xs, dtype=torch.int32).to(dev)
    return fn(q.to(dev), kc.to(dev), vc.to(dev), bt.to(dev), t(ctxs), t(qlens), scale)


def ref64_rows(q, kc, vc, bt_row, hist, scale):
    """fp64 oracle of one sequence: q [n,H,D] -> [n,H,D], row i judged by
    paged_decode_attn_ref64 with ctx = hist + i + 1."""
    n = q.shape[0]
    ctx = torch.arange(hist + 1, hist + n + 1, dtype=torch.int32)
    return ko.paged_decode_attn_ref64(q, kc, vc, bt_row.unsqueeze(0).expand(n, -1),
                                      ctx, scale)


def check_scatter_agrees(gen):
    """The scatter construction against the decode oracle: the contiguous
    fp64 reference and the paged one see the same numbers (<= 1e-15)."""
    c = ko.make_prefill_case(gen, "diffuse", 1, 2, 1, 80)
    kc, vc, bt, _ = scatter_paged(gen, c["k"], c["v"])
    ref = ko.attn_prefill_ref64(c["q"], c["k"], c["v"], c["scale"])   # [1,H,S,D]
    got = ref64_rows(c["q"][0].transpose(0, 1).contiguous(), kc, vc, bt[0], 0, c["scale"])
    assert float((got - ref[0].transpose(0, 1)).abs().max()) <= 1e-15


def check_pointer(fn, dev, gen, ctx, q_len, tmap):
    """Every real row equals expected[..., hist+i, :] bit for bit."""
    hist = ctx - q_len
    for B, H, Hk in HEAD_CONFIGS:
        c = ko.make_pointer_case(gen, B, H, Hk, ctx, tmap)
        gap = ko.pointer_min_gap(c["q"], c["k"], c["t"], c["scale"])
        assert gap >= ko.POINTER_MIN_GAP, f"generator: score gap {gap}"
        kc, vc, bt, _ = scatter_paged(gen, c["k"], c["v"])
        got = call(fn, dev, tail_rows(c["q"], q_len), kc, vc, bt,
                   [ctx] * B, [q_len] * B, c["scale"])
        what = f"paged pointer {tmap} ctx={ctx} q={q_len} B={B} H={H} Hk={Hk}"
        assert tuple(got.shape) == (B, q_len, H, ko.PREFILL_D), what
        ko.assert_bits_equal(got, tail_rows(c["expected"], q_len), what)
    assert hist >= 0


def check_future_decoy(fn, dev, gen, ctx, q_len):
    """Row i's strongest key is new token i+1, which IS in the cache.  The
    premises of ko.check_future_decoy, restricted to the rows hist.. ."""
    hist, S = ctx - q_len, ctx
    ratios = []
    for B, H, Hk in HEAD_CONFIGS:
        c = ko.make_decoy_case(gen, B, H, Hk, S)
        q, k, v = c["q"], c["k"], c["v"]
        kvh = ko.kv_head_of(H, Hk)
        assert S <= ko.PREFILL_S_MAX
        assert ko.max_abs_score_log2(q, k, c["scale"]) <= ko.SCORE_LOG2_MAX
        hidden = torch.ones(S, S, dtype=torch.bool).triu(1)
        if hist < S - 1:     # rows hist .. S-2 have a decoy
            for b in range(B):
                s = ko._scores64(q, k, c["scale"], b, torch.arange(H))
                decoy = s.diagonal(offset=1, dim1=1, dim2=2)[:, hist:]
                vis = s.masked_fill(hidden, float("-inf")).max(dim=2).values
                lead = float((decoy - vis[:, hist:S - 1]).min())
                assert lead >= ko.POINTER_MIN_GAP, f"generator: decoy leads by {lead}"
        ref = ko.attn_prefill_ref64(q, k, v, c["scale"])
        bound = ko.prefill_bound(v)
        lo = max(hist, 1)
        if lo < S - 1:
            leak = v[:, kvh].double()[:, :, lo + 1:]
            sep = (ref[:, :, lo:S - 1] - leak).abs().max(dim=-1).values
            assert float(sep.min()) > 4 * bound, "generator: a leak would pass"
        kc, vc, bt, _ = scatter_paged(gen, k, v)
        got = call(fn, dev, tail_rows(q, q_len), kc, vc, bt, [ctx] * B,
                   [q_len] * B, c["scale"])
        exp = tail_rows(ref, q_len)
        what = f"paged decoy ctx={ctx} q={q_len} B={B} H={H} Hk={Hk}"
        r = ko.err_ratio(got, exp, bound)
        print(f"{what}: max err / bound = {r:.3f}")
        ko.assert_within(got, exp, bound, what)
        ratios.append(r)
    return max(ratios)


def make_random_case(gen, geoms, H, Hk, pad=0):
    """Random caches (ko.make_paged_case) and queries for sequences with the
    given (ctx, q_len) each; Sq = max q_len + pad."""
    ctxs = [g[0] for g in geoms]
    qlens = [g[1] for g in geoms]
    case = ko.make_paged_case(gen, ctxs, H, Hk)
    Sq = max(qlens) + pad
    q = ko.rand_bf16(gen, len(geoms), Sq, H, ko.PREFILL_D)
    return dict(q=q, kcache=case["kcache"], vcache=case["vcache"],
                block_table=case["block_table"], ctxs=ctxs, qlens=qlens,
                scale=case["scale"])


def check_random(fn, dev, gen, geoms, H, Hk):
    """Every real row of every head against the fp64 decode oracle within
    ko.prefill_bound; rows past q_len exactly zero."""
    c = make_random_case(gen, geoms, H, Hk)
    kc, vc, bt = c["kcache"], c["vcache"], c["block_table"]
    P = kc.shape[0]
    got = call(fn, dev, c["q"], kc, vc, bt, c["ctxs"], c["qlens"], c["scale"]).cpu()
    bound = ko.prefill_bound(vc)
    rep = H // Hk
    worst = 0.0
    for b, (ctx, n) in enumerate(geoms):
        assert ctx <= ko.PREFILL_S_MAX
        qb = c["q"][b, :n]                                   # [n,H,D]
        kk = kc.double().view(P * PAGE, Hk, -1)[ko.slots_of(bt[b], ctx)]
        s = torch.einsum("nhd,chd->nhc", qb.double(),
                         kk.repeat_interleave(rep, dim=1)) * c["scale"]
        assert float(s.abs().max()) * math.log2(math.e) <= ko.SCORE_LOG2_MAX
        ref = ref64_rows(qb, kc, vc, bt[b], ctx - n, c["scale"])
        what = f"paged random seq {b} ctx={ctx} q={n} H={H} Hk={Hk}"
        r = ko.err_ratio(got[b, :n], ref, bound)
        print(f"{what}: max err / bound = {r:.3f}")
        ko.assert_within(got[b, :n], ref, bound, what)
        worst = max(worst, r)
        pad_rows = got[b, n:]
        assert int(ko.bits(pad_rows).count_nonzero()) == 0, what + ": pad rows not +0"
    return worst


def check_pad_and_stale(fn, dev, gen, geoms, H, Hk):
    """Pad rows of q at the largest finite bf16 and every cache slot at a
    position >= ctx (the rest of the last page, unowned pages) at +-largest
    finite: bit-equal to the same call with those regions zero, and pad rows
    exactly zero."""
    c = make_random_case(gen, geoms, H, Hk, pad=5)
    kc, vc, bt = c["kcache"], c["vcache"], c["block_table"]
    P, _, _, D = kc.shape
    live = torch.zeros(P * PAGE, dtype=torch.bool)
    for b, (ctx, _) in enumerate(geoms):
        live[ko.slots_of(bt[b], ctx)] = True
    sign = (torch.randint(0, 2, (P * PAGE, Hk, D), generator=gen) * 2 - 1).float()
    outs = []
    for fill in (BF16_MAX, 0.0):
        q = c["q"].clone()
        for b, n in enumerate(c["qlens"]):
            q[b, n:] = fill
        kf, vf = kc.clone().view(P * PAGE, Hk, D), vc.clone().view(P * PAGE, Hk, D)
        kf[~live] = (sign[~live] * fill).to(BF16)
        vf[~live] = (-sign[~live] * fill).to(BF16)
        outs.append(call(fn, dev, q, kf.view_as(kc), vf.view_as(vc), bt, c["ctxs"],
                         c["qlens"], c["scale"]).cpu())
    what = f"paged pad/stale {geoms} H={H} Hk={Hk}"
    assert bool(torch.isfinite(outs[0].float()).all()), what
    ko.assert_bits_equal(outs[0], outs[1], what)
    for b, n in enumerate(c["qlens"]):
        assert int(ko.bits(outs[0][b, n:]).count_nonzero()) == 0, what + ": pad rows not +0"
