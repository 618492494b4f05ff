"""fp64 transformer oracle for LlamaModel and the scorer, the configurations
and weights that make wiring errors visible, and the case drivers shared by
test_model_oracle_cpu.py (the model's CPU path, premises, mutants) and
test_model_exactness_gpu.py (the HIP path).  No tests live here.

The oracle is a plain Llama / Mixtral forward written from the mathematics.
It reads the model's weight TENSORS only (``model.layers[i][...]``, ``embed``,
``final_norm``, ``lm_head``, ``cos_sin``; for quantized models the stored
bytes and scales, dequantized in fp64) and calls no function of
``senweaver_amd.ops``.

Two modes:

* ``rounded=False``: fp64 throughout — the exact value.
* ``rounded=True``: the same mathematics with one rounding wherever the
  device path materialises a tensor: bf16 at every kernel output (the
  projections, rope, the attention output, the bf16 residual of
  fused_add_rmsnorm, the norm output, SwiGLU, the router logits, the MoE
  combine), and e4m3-rowwise / MX quantization of the activations wherever
  ``_linear``, ``_moe_ffn_fp8`` or ``logits`` quantize, by the fp64 quantizer
  rules of kernel_oracles.  Expert choice is taken from the exact pass, so
  the difference of the two modes holds rounding noise and no routing flips.
  ``p_bf16=True`` also rounds P to bf16 before the PV product inside
  attention, as the prefill kernels do (P is an MFMA operand; the row sum
  stays unrounded; decode rows keep P in fp32).  The drivers switch it on
  for a model on the GPU and off for the CPU path, whose reference
  attention keeps P in fp32 (measured effect on the MI355X: KERNELS.md).

The comparison metric, per token row::

    noise_row = || rounded - exact ||_2      err_row = || device - exact ||_2
    check:  err_row <= 2 * noise_row

Both sides of the bound come from the oracle alone.  The device rounds the
same quantities at the same points, so most of its roundings fall as the
rounded oracle's do and the typical ratio is 1.0; it parts from the oracle
where fp32 accumulation in another order tips a value over a rounding
boundary, and inside attention (online softmax, P as a bf16 MFMA operand).
With peaked softmaxes a few such differences can dominate a row, and the
factor 2 is the margin between two realisations of that process: measured
worst ratios are 1.0 .. 1.8 (KERNELS.md), while a wiring error moves
a row by 10 .. 65 noise norms (test_model_oracle_cpu.py).
"""

from __future__ import annotations

import math

import torch

import kernel_oracles as ko
from senweaver_amd import ops
from senweaver_amd.engine.kvcache import PAGE_SIZE, PagedKVCache
from senweaver_amd.engine.prefix_plan import plan_from_tokens
from senweaver_amd.models.config import ModelConfig
from senweaver_amd.models.llama import LlamaModel

BF16 = torch.bfloat16
F64 = torch.float64
MARGIN = 2.0        # err_row <= MARGIN * noise_row
GAP_FACTOR = 4.0    # router gap >= GAP_FACTOR * router-logit noise


# --------------------------------------------------------------------------
# roundings
# --------------------------------------------------------------------------
def r16(v: torch.Tensor) -> torch.Tensor:
    """bf16 round-to-nearest-even of fp64 values, back in fp64.  Magnitudes
    below 2^-120 (softmax weights of far keys) flush to zero: they are below
    anything a kernel output keeps."""
    v = torch.where(v.abs() < 2.0 ** -120, torch.zeros_like(v), v)
    return ko.bf16_rne64(v).double()


def _ident(v: torch.Tensor) -> torch.Tensor:
    return v


def act_quant64(x: torch.Tensor, quant: str) -> torch.Tensor:
    """Quantize-dequantize bf16-valued fp64 activations [..., K] by the rule
    of ops.quant_fp8 (f32 amax / 448 per row, RNE to e4m3) or ops.quant_mxfp8
    (power-of-two scale per 32 elements)."""
    K = x.shape[-1]
    x2 = x.reshape(-1, K)
    xb = x2.to(BF16)
    assert torch.equal(xb.double(), x2), "activation is not bf16-valued"
    if quant == "fp8":
        s = ko.quant_fp8_scale_ref(xb).double().unsqueeze(1)
        q = ko.e4m3_rne_bytes(x2 / s)
        return (ko.e4m3_to_f64(q) * s).reshape(x.shape)
    q, s = ko.quant_mxfp8_expect(xb)
    return ko.dequant_mx_ref64(q, s).reshape(x.shape)


# --------------------------------------------------------------------------
# weights
# --------------------------------------------------------------------------
def weight64(model, holder: dict, name: str) -> torch.Tensor:
    """fp64 [N, K] (or [E, N, K]) of a projection: the bf16 tensor, or the
    stored e4m3 bytes times their scales."""
    if name in holder:
        return holder[name].detach().cpu().double()
    q = holder[name + "_q"].detach().cpu()
    s = holder[name + "_s"].detach().cpu()
    K = q.shape[-1]
    q2 = q.reshape(-1, K)
    if model.quant == "fp8":
        w = ko.dequant_fp8_ref64(q2, s.reshape(-1))
    else:
        w = ko.dequant_mx_ref64(q2, s.reshape(-1, K // 32))
    return w.reshape(q.shape)


def lm_head64(model) -> torch.Tensor:
    if model.quant == "bf16":
        return model.lm_head.detach().cpu().double()
    return weight64(model, {"lm_head_q": model.lm_head_q,
                            "lm_head_s": model.lm_head_s}, "lm_head")


def _linear64(x, w64, quant, rounded, rows_q=None):
    """x [..., K] @ w^T.  In rounded mode on a quantized model the
    activation is quantized first; ``rows_q`` (bool, x's leading shape)
    restricts that to some rows (decode rows go through the GEMV kernels,
    which take bf16 activations)."""
    if rounded and quant != "bf16":
        xq = act_quant64(x, quant)
        x = xq if rows_q is None else torch.where(rows_q.unsqueeze(-1), xq, x)
    return x @ w64.t()


# --------------------------------------------------------------------------
# building blocks
# --------------------------------------------------------------------------
def _rmsnorm64(x, w, eps):
    return x * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + eps) * w


def _swiglu64(gu, swap=False):
    K = gu.shape[-1] // 2
    g, u = gu[..., :K], gu[..., K:]
    if swap:
        g, u = u, g
    return g * torch.sigmoid(g) * u


def _rope64(x, cos_sin, pos):
    """x [B, S, H, D], pos [B, S] -> rotate-half rope, via ko.rope_ref64."""
    B, S, H, D = x.shape
    out, _ = ko.rope_ref64(x.reshape(B * S, H, D), cos_sin, pos.reshape(B * S))
    return out.reshape(B, S, H, D)


def _attention64(q, k, v, scale, kv_of, rnd, p_rows=None, mask_ge=False):
    """Causal softmax attention.  q [B,S,Hq,D], k/v [B,S,Hk,D]; head h reads
    kv head kv_of[h].  ``p_rows`` (bool [B,S]): query rows whose P is rounded
    to bf16 before the PV product.  Returns ([B,S,Hq,D], fp64 scores std over
    the visible (row, key) pairs)."""
    B, S, Hq, D = q.shape
    i = torch.arange(S)
    hidden = i.unsqueeze(0) > i.unsqueeze(1)            # key j > row i
    if mask_ge:                                         # mutant: row i hides key i
        hidden = i.unsqueeze(0) >= i.unsqueeze(1)
        hidden[0, 0] = False
    out = torch.empty(B, S, Hq, D, dtype=F64)
    ssum = ssq = 0.0
    step = max(1, (1 << 24) // (Hq * S * S))
    for b0 in range(0, B, step):
        qq = q[b0:b0 + step].permute(0, 2, 1, 3)          # [b,Hq,S,D]
        kk = k[b0:b0 + step][:, :, kv_of].permute(0, 2, 1, 3)
        vv = v[b0:b0 + step][:, :, kv_of].permute(0, 2, 1, 3)
        s = (qq @ kk.transpose(-1, -2)) * scale
        vis = s[..., ~hidden]
        ssum += float(vis.sum())
        ssq += float((vis * vis).sum())
        s = s.masked_fill(hidden, float("-inf"))
        p = torch.exp(s - s.amax(dim=-1, keepdim=True))
        l = p.sum(dim=-1, keepdim=True)
        if p_rows is not None:
            p = torch.where(p_rows[b0:b0 + step, None, :, None], r16(p), p)
        out[b0:b0 + step] = rnd((p @ vv) / l).permute(0, 2, 1, 3)
    n = B * Hq * int((~hidden).sum())
    std = math.sqrt(max(ssq / n - (ssum / n) ** 2, 0.0))
    return out, std


def moe_slot_outputs64(model, L, h, choice, rounded=False, mutant=None, rows_q=None):
    """[T, k, H]: the SwiGLU FFN of expert choice[t, j] applied to h[t]."""
    c = model.config
    rnd = r16 if rounded else _ident
    w13, w2 = weight64(model, L, "w13"), weight64(model, L, "w2")
    present = sorted(set(choice.reshape(-1).tolist()))
    out = torch.zeros(h.shape[0], choice.shape[1], c.hidden_size, dtype=F64)
    for rank, e in enumerate(present):
        we = rank if mutant == "expert_by_rank" else e
        t, j = (choice == e).nonzero(as_tuple=True)
        rq = None if rows_q is None else rows_q[t]
        gu = rnd(_linear64(h[t], w13[we], model.quant, rounded, rq))
        act = rnd(_swiglu64(gu, swap=(mutant == "gate_up_swap")))
        out[t, j] = rnd(_linear64(act, w2[we], model.quant, rounded, rq))
    return out


def moe_ffn64(model, L, h, rounded=False, choice=None, mutant=None, rows_q=None):
    """Mixtral routed FFN on h [T, H] fp64: softmax -> top-k -> renormalise
    -> per-expert SwiGLU -> weighted sum.  ``choice`` [T, k] fixes the
    experts (the rounded pass takes the exact pass's).  Returns
    (out [T, H], router logits [T, E], choice [T, k], weights [T, k])."""
    k = model.config.num_experts_per_tok
    rnd = r16 if rounded else _ident
    logits = rnd(h @ L["router"].detach().cpu().double().t())
    probs = torch.softmax(logits, dim=-1)
    if choice is None:
        choice = probs.topk(k, dim=-1).indices
    w = probs.gather(1, choice)
    if mutant != "no_renorm":
        w = w / w.sum(dim=-1, keepdim=True)
    if mutant == "combine_order":   # weights permuted by order, not its inverse
        order = torch.argsort(choice.reshape(-1), stable=True)
        w = w.reshape(-1)[order][order].reshape(w.shape)
    d = moe_slot_outputs64(model, L, h, choice, rounded, mutant, rows_q)
    return rnd((w.unsqueeze(-1) * d).sum(dim=1)), logits, choice, w


class Forward:
    """Result of forward64.  hidden [B,S,H]; k / v: per layer [B,S,Hk,D]
    (K roped); router / choice: per MoE layer [B,S,E] / [B,S,k]; score_std,
    attn_ratio, ffn_ratio: per layer diagnostics of the premise tests (std
    of the visible attention scores in nats; mean row norm of the block
    output over that of the residual it is added to)."""

    def __init__(self):
        self.hidden = None
        self.k, self.v, self.router, self.choice = [], [], [], []
        self.score_std, self.attn_ratio, self.ffn_ratio = [], [], []


def _ratio(block, residual):
    return float((block.norm(dim=-1) / residual.norm(dim=-1)).mean())


def forward64(model, tokens, real_lens=None, rounded=False, choice=None,
              decode_from=None, decode_quant=True, mutant=None,
              p_bf16=False) -> Forward:
    """tokens [B, S] -> Forward.  Row b holds ``real_lens[b]`` meaningful
    positions (default S).  Attention is causal, so the pad positions after
    them change nothing before them; their hidden rows come back NaN, so a
    comparison that reaches into them fails.

    ``choice``: per MoE layer [B,S,k] expert ids (rounded mode: the exact
    pass's).  ``decode_from[b]``: positions >= it are decode steps; with
    ``decode_quant=False`` their projections take unquantized activations
    (the GEMV kernels).  ``mutant`` plants one wiring error."""
    c = model.config
    tok = tokens.detach().cpu().long()
    B, S = tok.shape
    Hq, Hk, D = c.num_heads, c.num_kv_heads, c.head_dim
    rep = Hq // Hk
    rnd = r16 if rounded else _ident
    quant = model.quant
    cos_sin = model.cos_sin.detach().cpu()
    pos = torch.arange(S).unsqueeze(0).expand(B, S)     # 0..S-1 per row
    qpos = kpos = pos
    if mutant == "pos_zero":
        qpos = kpos = torch.zeros_like(pos)
    rows_q = None
    p_rows = torch.ones(B, S, dtype=torch.bool) if rounded and p_bf16 else None
    if decode_from is not None:
        start = torch.tensor(decode_from).unsqueeze(1)
        if p_rows is not None:      # the decode kernel keeps P in fp32
            p_rows = pos < start
        if not decode_quant:
            rows_q = pos < start
        if mutant == "decode_pos_off":   # query one past the cached keys
            qpos = pos + (pos >= start).long()
    kv_of = torch.arange(Hq) // rep
    if mutant == "kv_mod":
        kv_of = torch.arange(Hq) % Hk
    n_in, n_post = "input_norm", "post_norm"
    if mutant == "norm_swap":
        n_in, n_post = n_post, n_in

    def normw(t):
        return t.detach().cpu().double()

    out = Forward()
    x = model.embed.detach().cpu().double()[tok]         # [B, S, H]
    residual = None
    for li, L in enumerate(model.layers):
        residual = x if residual is None else rnd(x + residual)
        h = rnd(_rmsnorm64(residual, normw(L[n_in]), c.rms_eps))
        qkv = rnd(_linear64(h, weight64(model, L, "qkv"), quant, rounded, rows_q))
        q = qkv[..., :c.q_size].reshape(B, S, Hq, D)
        k = qkv[..., c.q_size:c.q_size + c.kv_size].reshape(B, S, Hk, D)
        v = qkv[..., c.q_size + c.kv_size:].reshape(B, S, Hk, D)
        q = rnd(_rope64(q, cos_sin, qpos))
        if mutant != "k_unroped":
            k = rnd(_rope64(k, cos_sin, kpos))
        out.k.append(k)
        out.v.append(v)
        attn, std = _attention64(q, k, v, model.scale, kv_of, rnd, p_rows,
                                 mask_ge=(mutant == "mask_ge"))
        out.score_std.append(std)
        if mutant == "o_dh_order":       # heads concatenated [D, H]
            attn = attn.transpose(2, 3)
        o = rnd(_linear64(attn.reshape(B, S, Hq * D), weight64(model, L, "o"),
                          quant, rounded, rows_q))
        out.attn_ratio.append(_ratio(o, residual))
        if mutant == "res_before_norm":  # the norm sees the block output alone
            h = rnd(_rmsnorm64(o, normw(L[n_post]), c.rms_eps))
            residual = rnd(o + residual)
        else:
            residual = rnd(o + residual)
            h = rnd(_rmsnorm64(residual, normw(L[n_post]), c.rms_eps))
        if c.num_experts == 0:
            gu = rnd(_linear64(h, weight64(model, L, "gateup"), quant, rounded, rows_q))
            act = rnd(_swiglu64(gu, swap=(mutant == "gate_up_swap")))
            x = rnd(_linear64(act, weight64(model, L, "down"), quant, rounded, rows_q))
        else:
            ch = None if choice is None else choice[li].reshape(B * S, -1)
            rq = None if rows_q is None else rows_q.reshape(B * S)
            y, lg, ch, _ = moe_ffn64(model, L, h.reshape(B * S, -1), rounded, ch,
                                     mutant, rq)
            x = y.reshape(B, S, -1)
            out.router.append(lg.reshape(B, S, -1))
            out.choice.append(ch.reshape(B, S, -1))
        out.ffn_ratio.append(_ratio(x, residual))
    residual = rnd(x + residual)
    out.hidden = rnd(_rmsnorm64(residual, normw(model.final_norm), c.rms_eps))
    if real_lens is not None:
        for b, n in enumerate(real_lens):
            out.hidden[b, n:] = float("nan")
    return out


def logits64(model, hidden, rounded=False, act_quant=True) -> torch.Tensor:
    """lm_head logits of hidden [..., H] fp64.  Rounded: the activation
    quantized as ``LlamaModel.logits`` does (``act_quant=False``: the
    quantized-weight GEMV of small decode batches), bf16 output."""
    w = lm_head64(model)
    if not rounded:
        return hidden @ w.t()
    quant = model.quant if act_quant else "bf16"
    return r16(_linear64(hidden, w, quant, True))


# --------------------------------------------------------------------------
# the check
# --------------------------------------------------------------------------
def row_ratio(dev, exact, rounded) -> torch.Tensor:
    """err_row / noise_row over the last dim."""
    d = dev.detach().cpu().double()
    assert d.shape == exact.shape == rounded.shape, (d.shape, exact.shape)
    err = (d - exact).norm(dim=-1)
    noise = (rounded - exact).norm(dim=-1)
    return err / noise


def check_rows(dev, exact, rounded, what: str) -> float:
    """err_row <= 2 noise_row on every row (NaN fails).  Returns and prints
    the worst ratio."""
    r = row_ratio(dev, exact, rounded).reshape(-1)
    worst = float(r.max()) if bool(torch.isfinite(r).all()) else float("nan")
    print(f"{what}: worst err/noise = {worst:.3f} over {r.numel()} rows "
          f"(median {float(r.median()):.3f})")
    ok = r <= MARGIN
    assert bool(ok.all()), (f"{what}: {int((~ok).sum())} of {r.numel()} rows beyond "
                            f"{MARGIN} x noise; worst ratio {worst:.3f} at row "
                            f"{int((~ok).nonzero()[0])}")
    return worst


def rejected(mut, exact, rounded) -> torch.Tensor:
    """Per row: would check_rows refuse ``mut`` standing in for the device?"""
    return ~(row_ratio(mut, exact, rounded) <= MARGIN)


# --------------------------------------------------------------------------
# configurations and weights
# --------------------------------------------------------------------------
VOCAB = 512
MAXPOS = 512


def cfg_small(tie=False, layers=2, heads=6, kv_heads=2) -> ModelConfig:
    """q_size 768 != hidden 256, rep 3: the padded-tile paths."""
    return ModelConfig(name="oracle-small", hidden_size=256, intermediate_size=512,
                       num_layers=layers, num_heads=heads, num_kv_heads=kv_heads,
                       head_dim=128, vocab_size=VOCAB, max_position=MAXPOS,
                       tie_embeddings=tie)


def cfg_gemv(tie=False) -> ModelConfig:
    """Every projection K a multiple of 1024: decode reaches the GEMV kernels."""
    return ModelConfig(name="oracle-gemv", hidden_size=1024, intermediate_size=1024,
                       num_layers=2, num_heads=8, num_kv_heads=2, head_dim=128,
                       vocab_size=VOCAB, max_position=MAXPOS, tie_embeddings=tie)


def cfg_moe() -> ModelConfig:
    return ModelConfig(name="oracle-moe", hidden_size=256, intermediate_size=512,
                       num_layers=2, num_heads=6, num_kv_heads=2, head_dim=128,
                       vocab_size=VOCAB, max_position=MAXPOS, num_experts=4,
                       num_experts_per_tok=2)


# The random init hides wiring errors: norm weights of one, and scores of
# std 0.1 nat (near-uniform softmax, where rope and the mask move the output
# less than a bf16 rounding).  Targets of the rescale, for weights of std
# 0.02 and activations of rms ~1.04 after a norm with weights in [0.5, 1.5]:
Q_RMS = 2.1      # q, k element rms -> scores of std ~ Q_RMS^2 >= 4 nats
V_RMS = 1.0
GU_RMS = 1.6     # gate / up element rms
ROUTER_SCALE = 4.0
NORM_RMS = 1.04


def rescale_weights_(model: LlamaModel, seed: int = 7) -> None:
    """In place, on a bf16 model: norm weights random in [0.5, 1.5] (another
    draw per layer), the embedding to unit rms, q / k rows up until the
    scores have std >= 4 nats, the other projections so that every block's
    output is comparable in norm to the residual it is added to."""
    assert model.quant == "bf16"
    c = model.config
    g = torch.Generator().manual_seed(seed)
    std = 0.02

    def norm_(t):
        t.copy_((0.5 + torch.rand(t.shape, generator=g)).to(t.dtype))

    def scale_(t, f):
        t.copy_((t.float() * f).to(t.dtype))

    fan = std * math.sqrt(c.hidden_size) * NORM_RMS   # rms of x @ w^T, unit scale
    scale_(model.embed, 1.0 / std)
    if not c.tie_embeddings:
        scale_(model.lm_head, 4.0 / fan)              # logits of std ~4
    norm_(model.final_norm)
    for L in model.layers:
        norm_(L["input_norm"])
        norm_(L["post_norm"])
        qk = c.q_size + c.kv_size
        scale_(L["qkv"][:qk], Q_RMS / fan)
        scale_(L["qkv"][qk:], V_RMS / fan)
        scale_(L["o"], 1.0 / (std * math.sqrt(c.q_size) * V_RMS))
        act_rms = 0.45 * GU_RMS * GU_RMS              # rms of silu(g) u, roughly
        down = 1.0 / (std * math.sqrt(c.intermediate_size) * act_rms)
        if c.num_experts:
            scale_(L["router"], ROUTER_SCALE)
            scale_(L["w13"], GU_RMS / fan)
            scale_(L["w2"], down)
        else:
            scale_(L["gateup"], GU_RMS / fan)
            scale_(L["down"], down)


def build_model(cfg: ModelConfig, quant: str = "bf16", device="cpu",
                seed: int = 0) -> LlamaModel:
    """A model whose weights are the CPU-seeded init, rescaled, whatever the
    device (so the committed MoE tokens meet the same weights everywhere).
    Quantized models are re-quantized from the rescaled bf16 weights with
    ops.quant_* on the CPU; norm weights are not quantized."""
    src = LlamaModel(cfg, device="cpu", seed=seed)
    rescale_weights_(src)
    if quant == "bf16" and torch.device(device).type == "cpu":
        return src
    dst = LlamaModel(cfg, device=device, seed=seed, quant=quant)
    qfn = ops.quant_fp8 if quant == "fp8" else ops.quant_mxfp8

    def put(holder_dst, name, w):
        if name in holder_dst:
            holder_dst[name].copy_(w)
            return
        q, s = qfn(w)
        holder_dst[name + "_q"].copy_(q.reshape(holder_dst[name + "_q"].shape))
        holder_dst[name + "_s"].copy_(s.reshape(holder_dst[name + "_s"].shape))

    dst.embed.copy_(src.embed)
    dst.final_norm.copy_(src.final_norm)
    if quant == "bf16":
        if not cfg.tie_embeddings:
            dst.lm_head.copy_(src.lm_head)
    else:
        if not cfg.tie_embeddings:
            dst.lm_head.copy_(src.lm_head)
        q, s = qfn(src.lm_head)
        dst.lm_head_q.copy_(q)
        dst.lm_head_s.copy_(s)
    for Ls, Ld in zip(src.layers, dst.layers):
        for name, w in Ls.items():
            put(Ld, name, w)
    return dst


REAL_LENS = [37, 100]                                   # cache / decode cases
FORCED = torch.tensor([[5, 300, 77], [410, 9, 256]])    # teacher-forced ids


def dense_tokens(B: int, S: int, seed: int = 11) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, VOCAB, (B, S), generator=g)


# --------------------------------------------------------------------------
# MoE tokens: chosen so that no token's routing is ambiguous
# --------------------------------------------------------------------------
MOE_S = 64
MOE_CANDIDATES = 24
MOE_SEARCH_SEED = 4242


def router_gap_over_noise(ex: Forward, rd: Forward, k: int) -> torch.Tensor:
    """min over MoE layers of (k-th minus (k+1)-th exact router logit) over
    the row's router-logit noise max_e |rounded - exact|, [B, S]."""
    m = None
    for le, lr in zip(ex.router, rd.router):
        s = le.sort(dim=-1, descending=True).values
        r = (s[..., k - 1] - s[..., k]) / (lr - le).abs().amax(dim=-1)
        m = r if m is None else torch.minimum(m, r)
    return m


P_SETTINGS = (False, True)   # the rounded oracle of the CPU path / of the GPU


def search_moe_tokens(model, seq: int, S: int = MOE_S, N: int = MOE_CANDIDATES,
                      p_settings=P_SETTINGS) -> list:
    """Sequence ``seq`` picked left to right for one model: at position t, N
    random candidates as a batch sharing the prefix; kept is the candidate
    whose row t has the largest gap / noise (router_gap_over_noise), the
    minimum taken over the MoE layers and over the rounded oracles of
    ``p_settings``.  (Ranking by gap / spread alone left rows of the
    quantized models under the 4 x noise premise: their router noise varies
    several-fold from row to row.)"""
    g = torch.Generator().manual_seed(MOE_SEARCH_SEED + seq)
    k = model.config.num_experts_per_tok
    ids = []
    for t in range(S):
        cand = torch.randint(0, VOCAB, (N,), generator=g)
        toks = torch.cat([torch.tensor(ids, dtype=torch.long).expand(N, t),
                          cand.unsqueeze(1)], dim=1)
        ex = forward64(model, toks)
        ratio = None
        for p in p_settings:
            rd = forward64(model, toks, rounded=True, choice=ex.choice, p_bf16=p)
            r = router_gap_over_noise(ex, rd, k)[:, t]
            ratio = r if ratio is None else torch.minimum(ratio, r)
        ids.append(int(cand[int(ratio.argmax())]))
    return ids


# Chosen by search_moe_tokens(model, seq) for seq = 0, 1 on the fp8 and on
# the mxfp8 model (their weights, hence their routers' inputs, differ by the
# quantization); the bf16 model takes the fp8 model's tokens, where its own
# gaps are >= 9 x its noise.
MOE_TOKENS = {
    "fp8": [
        [162, 409, 265, 493, 424, 95, 55, 12, 346, 168, 208, 236, 430, 61, 401, 257,
         420, 425, 203, 332, 74, 385, 374, 265, 122, 206, 478, 463, 81, 371, 460, 481,
         332, 168, 5, 230, 389, 389, 420, 260, 451, 221, 388, 371, 424, 427, 318, 19,
         454, 50, 75, 122, 55, 388, 458, 72, 481, 231, 221, 231, 380, 273, 221, 462],
        [420, 493, 203, 89, 203, 496, 146, 14, 474, 14, 190, 100, 173, 123, 490, 454,
         98, 92, 437, 287, 144, 219, 273, 343, 464, 371, 82, 474, 145, 215, 202, 319,
         45, 441, 160, 469, 483, 390, 257, 82, 333, 326, 258, 3, 371, 493, 51, 323,
         24, 165, 132, 376, 403, 51, 469, 3, 511, 324, 355, 130, 464, 395, 65, 211],
    ],
    "mxfp8": [
        [494, 128, 490, 50, 258, 285, 480, 356, 33, 496, 329, 216, 430, 146, 337, 423,
         216, 121, 111, 480, 102, 102, 55, 459, 258, 206, 235, 445, 149, 24, 137, 108,
         283, 90, 71, 101, 26, 460, 106, 12, 403, 439, 388, 303, 142, 152, 396, 412,
         342, 360, 500, 157, 171, 95, 388, 375, 481, 226, 154, 41, 371, 344, 55, 179],
        [217, 432, 301, 266, 91, 229, 147, 14, 70, 413, 286, 302, 100, 345, 461, 275,
         191, 239, 356, 407, 434, 211, 420, 398, 379, 456, 504, 314, 144, 463, 76, 444,
         476, 439, 69, 105, 109, 48, 149, 199, 199, 393, 207, 125, 193, 30, 434, 280,
         194, 463, 469, 461, 140, 45, 454, 375, 511, 258, 154, 269, 112, 212, 6, 235],
    ],
}


def moe_tokens(quant: str) -> torch.Tensor:
    return torch.tensor(MOE_TOKENS["fp8" if quant == "bf16" else quant])


# --------------------------------------------------------------------------
# MoE layer cases: h constructed so that the routing is known
# --------------------------------------------------------------------------
def moe_layer_assignment(T: int) -> list:
    """(first, second) expert of every token.
    T=9: one pair for all, two experts empty (counts 0/9/0/9).
    T=130: one expert pair with exactly 1 row each, the other 129/129.
    T=300: counts 127/129/44/300 — both sides of a 128-row tile, a segment
    over several tiles; none a multiple of 16 (the fp8 path's padding)."""
    if T == 9:
        pairs = [(1, 3) if t % 2 else (3, 1) for t in range(T)]
    elif T == 130:
        pairs = [(0, 1)] + [(2, 3) if t % 2 else (3, 2) for t in range(1, T)]
    elif T == 300:
        first = [0] * 127 + [1] * 129 + [2] * 44
        pairs = [(e, 3) if t % 3 else (3, e) for t, e in enumerate(first)]
    else:
        raise ValueError(T)
    return pairs


MOE_LAYER_COUNTS = {9: [0, 9, 0, 9], 130: [1, 1, 129, 129], 300: [127, 129, 44, 300]}


def moe_layer_input(model, L, T: int, seed: int = 5) -> torch.Tensor:
    """h [T, H] bf16: a random part orthogonal to the router rows plus the
    combination of router rows that gives the first expert a logit in
    [0.45, 1.8], the second one 0 and the others -0.5: the first weight lies
    in [0.61, 0.86] and differs from token to token, the gap to the third
    expert is 0.5, and 14 .. 33% of the probability lies outside the top 2,
    several times the e4m3 noise, so a missing renormalisation shows."""
    c = model.config
    g = torch.Generator().manual_seed(seed + T)
    R = L["router"].detach().cpu().double()                      # [E, H]
    base = torch.randn(T, c.hidden_size, generator=g, dtype=F64)
    base = base - (base @ torch.linalg.pinv(R)) @ R              # R base^T = 0
    target = torch.full((T, c.num_experts), -0.5, dtype=F64)
    u = torch.rand(T, 2, generator=g, dtype=F64)
    for t, (e1, e2) in enumerate(moe_layer_assignment(T)):
        target[t, e1] = 0.45 + 1.35 * u[t, 0]
        target[t, e2] = 0.0
    coef = target @ torch.linalg.inv(R @ R.t())                  # (coef R) R^T = target
    return (base + coef @ R).to(BF16)


# --------------------------------------------------------------------------
# case drivers: run one path of the model on its device, compare with the
# oracle.  Each returns the worst err/noise ratio(s).
# --------------------------------------------------------------------------
def oracle_pair(model, tokens, **kw):
    """(exact, rounded) with the roundings of the model's device."""
    ex = forward64(model, tokens, **kw)
    rd = forward64(model, tokens, rounded=True, choice=ex.choice or None,
                   p_bf16=(model.device.type == "cuda"), **kw)
    return ex, rd


def run_prefill(model, tokens, what) -> float:
    ex, rd = oracle_pair(model, tokens)
    got = model.prefill(tokens.to(model.device))
    return check_rows(got, ex.hidden, rd.hidden, what)


def shuffled_cache(model, pages: int) -> PagedKVCache:
    """A cache filled with a sentinel whose next pages come out of order:
    two sequences are allocated and freed first."""
    cache = PagedKVCache(model.config, pages, model.device,
                         num_kv_heads=model.local_kv_heads)
    for t in cache.k + cache.v:
        t.fill_(ko.SENTINEL)
    a, b = cache.new_seq(), cache.new_seq()
    cache._ensure_capacity(a, 3 * PAGE_SIZE)
    cache._ensure_capacity(b, 2 * PAGE_SIZE)
    cache.free_seq(a)
    cache.free_seq(b)
    return cache


def _slots(cache, seq, n):
    return cache.slot_ids(seq, 0, n).cpu()


def run_prefill_cache(model, tokens, real_lens, what):
    """prefill(cache=...): hidden rows below real_len, the cached K (roped)
    and V of every layer through the block table, seq_lens, and the sentinel
    in every slot the prefill had no business writing.

    K and V rows are judged by the 2 x noise rule like the hidden rows.  V
    is not bit-equal to the rounded oracle's qkv slice (already on the CPU
    path some elements round the other way after fp32 accumulation: worst
    row ratio 1.03 in layer 0), and the pre-rope K of the device cannot be observed, so
    the elementwise bound of rope_ref64 has no input to apply to: it serves
    here as the oracle's rope."""
    c = model.config
    B, S = tokens.shape
    ex, rd = oracle_pair(model, tokens, real_lens=real_lens)
    cache = shuffled_cache(model, 24)
    seqs = [cache.new_seq() for _ in range(B)]
    got = model.prefill(tokens.to(model.device), cache=cache, seqs=seqs,
                        real_lens=real_lens)
    worst = {}
    for b, n in enumerate(real_lens):
        worst[f"hidden{b}"] = check_rows(got[b, :n], ex.hidden[b, :n],
                                         rd.hidden[b, :n], f"{what} hidden row {b}")
    assert [cache.seq_lens[s] for s in seqs] == list(real_lens)
    for b, s in enumerate(seqs):
        pages = cache.block_tables[s]
        assert pages != sorted(pages), "premise: page order is the identity"
    used = torch.zeros(cache.num_pages * PAGE_SIZE, dtype=torch.bool)
    P = cache.num_pages * PAGE_SIZE
    for li in range(c.num_layers):
        kf = cache.k[li].cpu().reshape(P, -1)
        vf = cache.v[li].cpu().reshape(P, -1)
        for b, n in enumerate(real_lens):
            sl = _slots(cache, seqs[b], n)
            used[sl] = True
            for nm, flat, e, r in (("K", kf, ex.k[li], rd.k[li]),
                                   ("V", vf, ex.v[li], rd.v[li])):
                worst[f"{nm}{li}.{b}"] = check_rows(
                    flat[sl], e[b, :n].reshape(n, -1), r[b, :n].reshape(n, -1),
                    f"{what} cached {nm} layer {li} row {b}")
        keep = torch.full_like(kf[~used], ko.SENTINEL)
        ko.assert_bits_equal(kf[~used], keep, f"{what} stray K write layer {li}")
        ko.assert_bits_equal(vf[~used], keep, f"{what} stray V write layer {li}")
    assert int((~used).sum()) >= sum((-n) % PAGE_SIZE for n in real_lens)
    return max(worst.values()), cache, seqs


def gemv_route(model) -> bool:
    """Do this model's decode-sized projections skip activation quantization
    (the quantized-weight GEMV kernels)?"""
    return model.device.type == "cuda" and model.config.hidden_size % 1024 == 0


def decode_sequences(tokens, real_lens, forced):
    """[B, max(real) + steps]: prompt[:real_len] then the forced tokens."""
    B = tokens.shape[0]
    steps = forced.shape[1]
    full = torch.zeros(B, max(real_lens) + steps, dtype=torch.long)
    for b, n in enumerate(real_lens):
        full[b, :n] = tokens[b, :n]
        full[b, n:n + steps] = forced[b]
    return full


def run_decode(model, tokens, real_lens, forced, mode, what, mutant=None):
    """Prefill into a shuffled cache, then ``forced`` [B, steps] teacher-
    forced through decode_step ('eager'), DecodeGraph.step_batch ('graph') or
    DecodeGraph.step ('graph1', B == 1).  Every step's hidden row and its
    logits against rows real_len + j of the oracle run over prompt + forced
    tokens.  With ``mutant`` the oracle mutant stands in for the device and
    the rejected rows are returned instead."""
    B, steps = forced.shape
    full = decode_sequences(tokens, real_lens, forced)
    dq = not gemv_route(model)
    kw = dict(real_lens=[n + steps for n in real_lens], decode_from=list(real_lens),
              decode_quant=dq)
    ex, rd = oracle_pair(model, full, **kw)
    rows = [(b, n + j) for j in range(steps) for b, n in enumerate(real_lens)]
    bi = torch.tensor([r[0] for r in rows])
    si = torch.tensor([r[1] for r in rows])
    eh, rh = ex.hidden[bi, si], rd.hidden[bi, si]
    el, rl = logits64(model, eh), logits64(model, rh, rounded=True, act_quant=dq)
    if mutant is not None:
        mh = forward64(model, full, mutant=mutant, **kw).hidden[bi, si]
        return rejected(mh, eh, rh)
    dev = model.device
    cache = shuffled_cache(model, 24)
    seqs = [cache.new_seq() for _ in range(B)]
    model.prefill(tokens.to(dev), cache=cache, seqs=seqs, real_lens=list(real_lens))
    graph = None
    if mode != "eager":
        from senweaver_amd.engine.graph import DecodeGraph
        graph = DecodeGraph(model, cache, 24, batch=B)
    hs, ls = [], []
    for j in range(steps):
        if mode == "eager":
            pos = torch.tensor([cache.seq_lens[s] for s in seqs], device=dev)
            h = model.decode_step(forced[:, j].to(dev), pos, cache, seqs)
        elif mode == "graph":
            h = graph.step_batch(forced[:, j].tolist(), seqs)
        else:
            assert B == 1
            h = graph.step(int(forced[0, j]), seqs[0])
        hs.append(h.clone())
        ls.append(model.logits(h))
    assert [cache.seq_lens[s] for s in seqs] == [n + steps for n in real_lens]
    wh = check_rows(torch.cat(hs), eh, rh, f"{what} hidden")
    wl = check_rows(torch.cat(ls), el, rl, f"{what} logits")
    return wh, wl


def run_extend(model, tokens, hist, new, what) -> float:
    """tokens [1, hist + new]: ``hist`` positions prefilled into a shuffled
    cache, then prefill_extend of the ``new`` ones, padded to 64 rows."""
    dev = model.device
    total = hist + new
    ex, rd = oracle_pair(model, tokens[:, :total])
    cache = shuffled_cache(model, 24)
    seq = cache.new_seq()
    S = (hist + 127) & ~127
    first = torch.zeros(1, S, dtype=torch.long)
    first[0, :hist] = tokens[0, :hist]
    model.prefill(first.to(dev), cache=cache, seqs=[seq], real_lens=[hist])
    Sq = (new + 63) & ~63
    ext = torch.zeros(1, Sq, dtype=torch.long)
    ext[0, :new] = tokens[0, hist:total]
    got = model.prefill_extend(ext.to(dev), cache, [seq], [new])
    assert cache.seq_lens[seq] == total
    return check_rows(got[0, :new], ex.hidden[0, hist:total],
                      rd.hidden[0, hist:total], what)


def run_moe_layer(model, T, what) -> float:
    L = model.layers[0]
    h = moe_layer_input(model, L, T)
    ex, _, ch, w = moe_ffn64(model, L, h.double())
    counts = torch.bincount(ch.reshape(-1), minlength=model.config.num_experts)
    assert counts.tolist() == MOE_LAYER_COUNTS[T], f"premise: counts {counts.tolist()}"
    rd = moe_ffn64(model, L, h.double(), rounded=True, choice=ch)[0]
    got = model._moe_ffn(h.to(model.device), L)
    return check_rows(got, ex, rd, what)


# ---- scorer ----
SCORER_B, SCORER_S = 4, 128


def scorer_case(S: int = SCORER_S, seed: int = 23):
    """tokens, mask [4, S].  Rows share 0 / 64 / 70 / S tokens with the
    previous row.  Row 0: position 0 and the last position masked among
    others.  Row 1: zero-padded from position S - 28, its last real position
    masked.  Row 2: only position 0 masked — an empty mask once position 0
    is ignored, score 0.  Row 3: row 2's tokens, another mask."""
    g = torch.Generator().manual_seed(seed)
    B, tail = SCORER_B, S - 28
    tok = torch.randint(1, VOCAB, (B, S), generator=g)
    tok[1, :64] = tok[0, :64]
    tok[1, 64] = int(tok[0, 64]) % (VOCAB - 1) + 1
    tok[1, tail:] = 0
    tok[2, :70] = tok[1, :70]
    tok[2, 70] = int(tok[1, 70]) % (VOCAB - 1) + 1
    tok[3] = tok[2]
    mask = torch.zeros(B, S, dtype=torch.bool)
    mask[0] = torch.rand(S, generator=g) < 0.25
    mask[0, 0] = mask[0, S - 1] = True
    # rows 1 and 3: few positions, most of them inside the shared prefix, so
    # that a gather from the wrong packed rows is not averaged away
    mask[1, [10, 30, 50, tail - 1]] = True
    mask[2, 0] = True
    mask[3, [0, 7, 33, 60, S - 1]] = True
    return tok, mask


def score64(model, tokens, mask, ex: Forward, rd: Forward, mutant=None):
    """(expected [B], bound [B]).  Expected: mean over the masked positions
    p >= 1 of log_softmax(logits64(hidden[p-1]))[tokens[p]], 0 for an empty
    mask.  Bound: 2 x the mean over those positions of
    2 max_v |logit_rounded - logit_exact| (log-softmax is 2-Lipschitz in the
    sup norm; the outer 2 is the margin of the row check)."""
    B, S = tokens.shape
    m = mask.clone()
    if mutant != "keep_pos0":
        m[:, 0] = False
    flat = m.reshape(-1).nonzero().squeeze(1)
    src = flat if mutant == "target_at_p" else flat - 1    # -1 wraps, as torch does
    src = src % (B * S)
    if mutant == "own_rows_in_prefix":
        plan = plan_from_tokens(tokens.tolist())
        stored = plan.stored_tokens()
        b, s = src // S, src % S
        packed = [plan.base[int(bb)] + int(ss) for bb, ss in zip(b, s)]
        src = torch.tensor([stored[r][0] * S + stored[r][1] for r in packed])
    eh = ex.hidden.reshape(B * S, -1)[src]
    le = logits64(model, eh)
    lr = logits64(model, rd.hidden.reshape(B * S, -1)[src], rounded=True)
    tgt = tokens.reshape(-1)[flat]
    lp = torch.log_softmax(le, dim=-1).gather(1, tgt.unsqueeze(1)).squeeze(1)
    dl = 2.0 * (lr - le).abs().amax(dim=-1)
    seq = flat // S
    n = torch.zeros(B, dtype=F64).index_add_(0, seq, torch.ones_like(lp))
    exp = torch.zeros(B, dtype=F64).index_add_(0, seq, lp) / n.clamp(min=1)
    bound = MARGIN * torch.zeros(B, dtype=F64).index_add_(0, seq, dl) / n.clamp(min=1)
    return exp, bound


def check_scores(got, exp, bound, what) -> float:
    err = (got.detach().cpu().double() - exp).abs()
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300),
                        torch.where(err > 0, float("inf"), 0.0).double())
    print(f"{what}: |score - expected| / bound = {[round(float(r), 3) for r in ratio]} "
          f"(bound already holds the margin {MARGIN})")
    assert bool((err <= bound).all()), f"{what}: err {err.tolist()} bound {bound.tolist()}"
    return float(ratio.max())


def run_scorer(model, prefix_pack, micro_batch, what, S=SCORER_S) -> float:
    from senweaver_amd.engine.scorer import LlamaBackend
    tok, mask = scorer_case(S)
    ex, rd = oracle_pair(model, tok)
    exp, bound = score64(model, tok, mask, ex, rd)
    assert float(exp[2]) == 0.0 and float(bound[2]) == 0.0
    be = LlamaBackend(model.config, device=str(model.device), prefix_pack=prefix_pack,
                      micro_batch=SCORER_B)
    be.model = model
    t, m = tok.to(model.device), mask.to(model.device)
    if micro_batch is None:
        got = be.score_token_batch_device(t, m)
    else:
        got = be.score_microbatches(t, m, micro_batch=micro_batch)
    return check_scores(got, exp, bound, what)
