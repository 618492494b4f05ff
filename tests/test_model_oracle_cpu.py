"""The fp64 model oracle of tests/model_oracle.py, proven on the CPU before a
GPU is touched:

* the oracle against an independent composition of ops.reference functions
  in fp32;
* every case of test_model_exactness_gpu.py through the same driver on the
  model's CPU path (same bound: err_row <= 2 noise_row);
* the premises the cases rest on: score std >= 4 nats, block / residual
  norm ratios, router gaps >= 4 x router noise with no flips for the
  committed MoE tokens, the token search reproducing them, the MoE-layer
  cases hitting their per-expert counts;
* mutants: the oracle with ONE wiring error standing in for the device must
  be refused by the same check — on >= 90% of the eligible rows at model
  level, on every row for the MoE-layer mutants (combine order: on every
  row it moves by more than 4 x the row's noise).

"Positions not restarting per batch row" is not among the mutants: rope is
relative, so a uniform shift of a row's q and k positions changes nothing in
a full prefill (and "+1" everywhere is invisible for the same reason).
"""

import pytest
import torch

import model_oracle as mo
from senweaver_amd.ops import reference as ref

QUANTS = ["bf16", "fp8", "mxfp8"]
REAL_LENS, FORCED = mo.REAL_LENS, mo.FORCED
_MODELS = {}


def model_of(key, cfg, quant="bf16"):
    if (key, quant) not in _MODELS:
        _MODELS[(key, quant)] = mo.build_model(cfg, quant, "cpu")
    return _MODELS[(key, quant)]


def small(quant="bf16"):
    return model_of("small", mo.cfg_small(), quant)


def gemv(quant="bf16"):
    return model_of("gemv", mo.cfg_gemv(), quant)


def moe(quant="bf16"):
    return model_of("moe", mo.cfg_moe(), quant)


# --------------------------------------------------------------------------
# the oracle against ops.reference in fp32
# --------------------------------------------------------------------------
def _ref_forward32(model, tokens):
    c = model.config
    B, S = tokens.shape
    T = B * S
    f = lambda t: t.float()
    pos = torch.arange(S).repeat(B)
    x = f(model.embed)[tokens.reshape(T)]
    res = torch.zeros_like(x)
    for L in model.layers:
        h, res = ref.fused_add_rmsnorm_ref(x, res, f(L["input_norm"]), c.rms_eps)
        qkv = ref.gemm_bt_ref(h, f(L["qkv"]))
        q = qkv[:, :c.q_size].reshape(T, c.num_heads, c.head_dim)
        k = qkv[:, c.q_size:c.q_size + c.kv_size].reshape(T, c.num_kv_heads, c.head_dim)
        v = qkv[:, c.q_size + c.kv_size:].reshape(B, S, c.num_kv_heads, c.head_dim)
        q = ref.rope_ref(q, model.cos_sin, pos).reshape(B, S, c.num_heads, c.head_dim)
        k = ref.rope_ref(k, model.cos_sin, pos).reshape(B, S, c.num_kv_heads, c.head_dim)
        a = ref.attn_fwd_ref(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
                             model.scale)
        o = ref.gemm_bt_ref(a.transpose(1, 2).reshape(T, c.q_size), f(L["o"]))
        h, res = ref.fused_add_rmsnorm_ref(o, res, f(L["post_norm"]), c.rms_eps)
        x = ref.gemm_bt_ref(ref.swiglu_ref(ref.gemm_bt_ref(h, f(L["gateup"]))),
                            f(L["down"]))
    h, _ = ref.fused_add_rmsnorm_ref(x, res, f(model.final_norm), c.rms_eps)
    return h.reshape(B, S, -1)


def test_oracle_matches_reference_composition():
    """fp32 accuracy: unit roundoff 6e-8, sums of up to 768 terms and a
    softmax over scores of up to ~30 nats — a relative row error of 1e-4
    leaves two decades; any wiring difference is O(1)."""
    m = small()
    tok = mo.dense_tokens(2, 128)
    ex = mo.forward64(m, tok)
    got = _ref_forward32(m, tok).double()
    rel = (got - ex.hidden).norm(dim=-1) / ex.hidden.norm(dim=-1)
    print(f"oracle vs fp32 composition: worst relative row error {float(rel.max()):.2e}")
    assert float(rel.max()) <= 1e-4
    lg = ref.gemm_bt_ref(got.float().reshape(-1, 256), m.lm_head.float()).double()
    l64 = mo.logits64(m, got.reshape(-1, 256))
    assert float(((lg - l64).norm(dim=-1) / l64.norm(dim=-1)).max()) <= 1e-5


# --------------------------------------------------------------------------
# the GPU file's cases on the model's CPU path
# --------------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 128, 192])
@pytest.mark.parametrize("quant", QUANTS)
def test_prefill_small_cpu(quant, S):
    mo.run_prefill(small(quant), mo.dense_tokens(2, S), f"prefill small {quant} S={S}")


def test_prefill_other_configs_cpu():
    mo.run_prefill(model_of("tied", mo.cfg_small(tie=True)), mo.dense_tokens(2, 128),
                   "prefill small tied")
    mo.run_prefill(gemv(), mo.dense_tokens(2, 128), "prefill gemv bf16 S=128")
    mo.run_prefill(model_of("wide128", mo.cfg_small(layers=1, heads=8)),
                   mo.dense_tokens(64, 128), "prefill B=64 S=128 H=8")
    mo.run_prefill(model_of("v5", mo.cfg_small(layers=1, heads=16, kv_heads=4)),
                   mo.dense_tokens(32, 256), "prefill B=32 S=256 H=16")


def test_prefill_into_cache_cpu():
    mo.run_prefill_cache(gemv(), mo.dense_tokens(2, 128), REAL_LENS, "prefill+cache gemv")


@pytest.mark.parametrize("quant", QUANTS)
def test_decode_cpu(quant):
    mo.run_decode(gemv(quant), mo.dense_tokens(2, 128), REAL_LENS, FORCED, "eager",
                  f"decode eager gemv {quant} B=2")
    mo.run_decode(gemv(quant), mo.dense_tokens(2, 128)[1:], REAL_LENS[1:], FORCED[1:],
                  "eager", f"decode eager gemv {quant} B=1")


def test_prefill_extend_cpu():
    mo.run_extend(gemv(), mo.dense_tokens(1, 137, seed=13), 100, 37,
                  "prefill_extend gemv 100+37")


@pytest.mark.parametrize("T", [9, 130, 300])
@pytest.mark.parametrize("quant", QUANTS)
def test_moe_layer_cpu(quant, T):
    mo.run_moe_layer(moe(quant), T, f"moe layer {quant} T={T}")


@pytest.mark.parametrize("quant", QUANTS)
def test_moe_model_cpu(quant):
    mo.run_prefill(moe(quant), mo.moe_tokens(quant), f"prefill moe {quant} S=64")


@pytest.mark.parametrize("micro_batch", [None, 2])
@pytest.mark.parametrize("prefix_pack", [True, False])
def test_scorer_cpu(prefix_pack, micro_batch):
    mo.run_scorer(small(), prefix_pack, micro_batch,
                  f"scorer pack={prefix_pack} micro_batch={micro_batch}")


def test_scorer_s256_cpu():
    mo.run_scorer(small(), True, None, "scorer pack=True S=256", S=256)


# --------------------------------------------------------------------------
# premises
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "tied", "gemv", "moe"])
def test_premise_scores_and_block_ratios(name):
    """Scores of std >= 4 nats in every layer (softmax far from uniform),
    and every block's output within a factor 4 of the residual it joins."""
    m = {"small": small, "gemv": gemv, "moe": moe,
         "tied": lambda: model_of("tied", mo.cfg_small(tie=True))}[name]()
    ex = mo.forward64(m, mo.dense_tokens(2, 128))
    print(name, ex.score_std, ex.attn_ratio, ex.ffn_ratio)
    assert min(ex.score_std) >= 4.0
    for r in ex.attn_ratio + ex.ffn_ratio:
        assert 0.25 <= r <= 4.0
    for L in m.layers:   # norm weights: in [0.5, 1.5], another draw per layer
        for n in ("input_norm", "post_norm"):
            assert 0.5 <= float(L[n].min()) and float(L[n].max()) <= 1.5
    ws = [L[n] for L in m.layers for n in ("input_norm", "post_norm")] + [m.final_norm]
    assert all(not torch.equal(a, b) for i, a in enumerate(ws) for b in ws[:i])


@pytest.mark.parametrize("p_bf16", mo.P_SETTINGS)
@pytest.mark.parametrize("quant", QUANTS)
def test_premise_router_gaps(quant, p_bf16):
    """Committed MoE tokens: in every MoE layer every token's gap between
    the 2nd and 3rd router logit is >= 4 x its router-logit noise, and the
    rounded oracle routes as the exact one — for the rounded oracle of the
    CPU path (P in fp32) and for the one the GPU tests use (P in bf16)."""
    m = moe(quant)
    k = m.config.num_experts_per_tok
    tok = mo.moe_tokens(quant)
    ex = mo.forward64(m, tok)
    rd = mo.forward64(m, tok, rounded=True, choice=ex.choice, p_bf16=p_bf16)
    worst = float(mo.router_gap_over_noise(ex, rd, k).min())
    print(f"router gap / noise {quant} p_bf16={p_bf16}: min {worst:.2f}")
    assert worst >= mo.GAP_FACTOR
    for le, lr, ch in zip(ex.router, rd.router, ex.choice):
        own = lr.topk(k, dim=-1).indices.sort(dim=-1).values
        assert torch.equal(own, ch.sort(dim=-1).values), "routing flip"
        counts = torch.bincount(ch.reshape(-1), minlength=m.config.num_experts)
        assert int(counts.min()) >= 16, f"unbalanced experts {counts.tolist()}"


@pytest.mark.parametrize("quant", ["fp8", "mxfp8"])
def test_premise_search_reproduces_tokens(quant):
    """The search re-run in full for one sequence of each token set."""
    assert mo.search_moe_tokens(moe(quant), 0) == mo.MOE_TOKENS[quant][0]


@pytest.mark.parametrize("T", [9, 130, 300])
@pytest.mark.parametrize("quant", QUANTS)
def test_premise_moe_layer_routing(quant, T):
    m = moe(quant)
    L = m.layers[0]
    h = mo.moe_layer_input(m, L, T).double()
    _, lg, ch, w = mo.moe_ffn64(m, L, h)
    counts = torch.bincount(ch.reshape(-1), minlength=4).tolist()
    assert counts == mo.MOE_LAYER_COUNTS[T]
    assert [tuple(r) for r in ch.tolist()] == mo.moe_layer_assignment(T)
    assert float(w.max(dim=-1).values.min()) >= 0.6, "top-2 weights too equal"
    s = lg.sort(dim=-1, descending=True).values
    assert float((s[:, 1] - s[:, 2]).min()) >= 0.45
    outside = 1.0 - torch.softmax(lg, dim=-1).gather(1, ch).sum(dim=-1)
    assert float(outside.min()) >= 0.12, "renormalisation would not show"


# --------------------------------------------------------------------------
# mutants
# --------------------------------------------------------------------------
MODEL_MUTANTS = ["kv_mod", "norm_swap", "k_unroped", "pos_zero", "mask_ge",
                 "res_before_norm", "gate_up_swap", "o_dh_order"]
_PAIR = {}


def _small_pair():
    if not _PAIR:
        tok = mo.dense_tokens(2, 128)
        _PAIR["tok"] = tok
        _PAIR["ex"], _PAIR["rd"] = mo.oracle_pair(small(), tok)
    return _PAIR["tok"], _PAIR["ex"], _PAIR["rd"]


@pytest.mark.parametrize("mutant", MODEL_MUTANTS)
def test_model_mutant_rejected(mutant):
    """Eligible rows: positions >= 1 (at position 0 rope is the identity and
    there is one key, so several mutants coincide with the model there)."""
    tok, ex, rd = _small_pair()
    mut = mo.forward64(small(), tok, mutant=mutant).hidden
    ratio = mo.row_ratio(mut, ex.hidden, rd.hidden)[:, 1:]
    frac = float(mo.rejected(mut, ex.hidden, rd.hidden)[:, 1:].double().mean())
    print(f"mutant {mutant}: rejected {frac:.3f}, median err/noise "
          f"{float(ratio.median()):.1f}")
    assert frac >= 0.9


def test_decode_position_mutant_rejected():
    rej = mo.run_decode(gemv(), mo.dense_tokens(2, 128), REAL_LENS, FORCED, "eager",
                        "decode mutant", mutant="decode_pos_off")
    assert float(rej.double().mean()) >= 0.9


def _layer_mutant(quant, T, mutant):
    """(rejected [T], own weights, mutant's weights, noise_row, d [T,k,H])."""
    m = moe(quant)
    L = m.layers[0]
    h = mo.moe_layer_input(m, L, T).double()
    ex, _, ch, w = mo.moe_ffn64(m, L, h)
    rd = mo.moe_ffn64(m, L, h, rounded=True, choice=ch)[0]
    mut, _, _, wm = mo.moe_ffn64(m, L, h, choice=ch, mutant=mutant)
    d = mo.moe_slot_outputs64(m, L, h, ch)
    return mo.rejected(mut, ex, rd), w, wm, (rd - ex).norm(dim=-1), d


@pytest.mark.parametrize("T", [9, 130, 300])
@pytest.mark.parametrize("quant", QUANTS)
def test_moe_layer_mutant_no_renorm(quant, T):
    rej = _layer_mutant(quant, T, "no_renorm")[0]
    assert bool(rej.all()), f"{int((~rej).sum())} rows accepted"


@pytest.mark.parametrize("quant", QUANTS)
def test_moe_layer_mutant_expert_by_rank(quant):
    """Visible where an expert is empty: the T=9 case (experts 0 and 2)."""
    rej = _layer_mutant(quant, 9, "expert_by_rank")[0]
    assert bool(rej.all())


MIN_WRONG = {9: 2, 130: 65, 300: 150}   # T=9 aside, at least half the rows


@pytest.mark.parametrize("T", [9, 130, 300])
@pytest.mark.parametrize("quant", QUANTS)
def test_moe_layer_mutant_combine_order(quant, T):
    """The permutation hands a row the weights of other rows; first weights
    lie in [0.61, 0.86], so a row may draw weights close to its own back and
    is then not a wrong row.  Whether a row is wrong is judged against its
    own noise: the weight shift max_j |dw_j| times || d_1 - d_2 || (the
    exact displacement when the two shifts are opposite) beyond twice the
    bound of the check, 4 x noise_row.  Every such row must be refused."""
    rej, w, wm, noise, d = _layer_mutant(quant, T, "combine_order")
    shift = (wm - w).abs().amax(dim=-1) * (d[:, 0] - d[:, 1]).norm(dim=-1)
    wrong = shift > 2 * mo.MARGIN * noise
    print(f"combine_order {quant} T={T}: {int(wrong.sum())} rows wrong, "
          f"{int(rej.sum())} refused")
    assert bool(rej[wrong].all())
    assert int(wrong.sum()) >= MIN_WRONG[T]


@pytest.mark.parametrize("mutant", ["target_at_p", "keep_pos0", "own_rows_in_prefix"])
def test_scorer_mutant_rejected(mutant):
    """The mutant's scores fail the GPU test's check, on the sequences the
    error can reach: keep_pos0 on the row whose mask is position 0 alone
    (expected exactly 0), own_rows_in_prefix on the rows that share a prefix
    and mask positions inside it, target_at_p on the rows 0 and 3."""
    m = small()
    tok, mask = mo.scorer_case()
    ex, rd = mo.oracle_pair(m, tok)
    exp, bound = mo.score64(m, tok, mask, ex, rd)
    mut, _ = mo.score64(m, tok, mask, ex, rd, mutant=mutant)
    rows = {"keep_pos0": [2], "own_rows_in_prefix": [1, 3], "target_at_p": [0, 3]}[mutant]
    err = (mut - exp).abs()
    print(f"scorer mutant {mutant}: err {err.tolist()} bound {bound.tolist()}")
    with pytest.raises(AssertionError):
        mo.check_scores(mut, exp, bound, f"mutant {mutant}")
    for b in rows:
        assert float(err[b]) > float(bound[b]), f"row {b} accepted"
