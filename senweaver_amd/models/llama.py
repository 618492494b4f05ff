"""Llama backbone on the senweaver_amd gfx950 kernel library.

Replaces the reference's remote LLM providers (sendLLMMessage.impl.ts's 20
HTTPS backends) with a local model whose fused and shape-special ops are
hand-written HIP: fused residual+RMSNorm, table-driven RoPE, flash prefill
attention, paged decode attention, SwiGLU, decode GEMV, fp8/mxfp8 GEMMs and
fused logit reductions.  Plain bf16 prefill projections go to hipBLASLt
through ``ops.gemm_bt`` (it measured faster than the in-repo tiled MFMA GEMM
at those shapes; SENWEAVER_GEMM=hip forces the in-repo kernel).  PyTorch
supplies tensor storage, reshapes/transposes and the embedding gather.

Weights are random-init bf16 (no network access for checkpoints — bench data
is declared synthetic).
"""

from __future__ import annotations

import math
import os
from typing import TYPE_CHECKING, Callable, List, Optional

import torch

from .. import ops
from .config import ModelConfig

if TYPE_CHECKING:  # avoids the engine<->models import cycle
    from ..engine.kvcache import PagedKVCache


class LlamaModel:
    def __init__(self, config: ModelConfig, device="cpu", dtype=torch.bfloat16, seed: int = 0,
                 tp=None, quant: str = "bf16", ep=None):
        from ..parallel.tp import TPContext, shard_gateup, shard_qkv, shard_rows
        from ..parallel.ep import EPContext
        self.config = config
        self.device = torch.device(device)
        self.dtype = dtype
        self.tp = tp if tp is not None else TPContext()
        # expert parallelism (parallel/ep.py): contiguous expert shards per
        # rank, all-to-all token routing.  Mutually exclusive with TP here
        # (BASELINE needs neither combined; the collectives would nest).
        self.ep = ep if ep is not None else EPContext()
        if self.ep.world > 1:
            assert config.num_experts % self.ep.world == 0
            # EP composes with TP (parallel/grid.py): experts sharded over
            # the EP group, each local expert TP-sharded like the dense FFN.
            # The quantized grouped-GEMM path is EP-unaware (global counts).
            assert quant == "bf16", "EP supports the bf16 expert path"
        c = config
        tpw = self.tp.world
        if tpw > 1:
            assert c.num_heads % tpw == 0 and c.num_kv_heads % tpw == 0, \
                f"TP={tpw} must divide heads ({c.num_heads}/{c.num_kv_heads})"
            assert c.intermediate_size % tpw == 0
        self.local_heads = c.num_heads // tpw
        self.local_kv_heads = c.num_kv_heads // tpw
        self.local_q_size = self.local_heads * c.head_dim
        self.local_kv_size = self.local_kv_heads * c.head_dim
        self.local_inter = c.intermediate_size // tpw
        assert quant in ("bf16", "fp8", "mxfp8")
        self.quant = quant
        if self.device.type == "cuda":
            # Device-side init: seconds for 8B instead of minutes of CPU RNG +
            # PCIe transfer.  Same seed + same call order on every rank =>
            # identical weights across the DP group (Philox is device-count
            # independent), which candidate-parallel scoring requires.
            gen = torch.Generator(device=self.device).manual_seed(seed)

            def W(*shape, std=0.02):
                t = torch.empty(shape, dtype=torch.float32, device=self.device)
                t.normal_(0.0, std, generator=gen)
                return t.to(dtype)
        else:
            g = torch.Generator(device="cpu").manual_seed(seed)

            def W(*shape, std=0.02):
                t = torch.empty(shape, dtype=torch.float32)
                t.normal_(0.0, std, generator=g)
                return t.to(dtype).to(self.device)

        self.embed = W(c.vocab_size, c.hidden_size)
        self.layers = []
        for _ in range(c.num_layers):
            # full weights are generated with the shared seed, then sliced to
            # this rank's shard: every TP degree sees the SAME model, and all
            # ranks agree by construction
            qkv_full = W(c.q_size + 2 * c.kv_size, c.hidden_size)
            o_full = W(c.hidden_size, c.q_size)
            layer = {
                "input_norm": torch.ones(c.hidden_size, dtype=dtype, device=self.device),
                "qkv": shard_qkv(qkv_full, c.num_heads, c.num_kv_heads, c.head_dim, self.tp)
                        if tpw > 1 else qkv_full,
                "o": shard_rows(o_full, self.tp, dim=1) if tpw > 1 else o_full,
                "post_norm": torch.ones(c.hidden_size, dtype=dtype, device=self.device),
            }
            del qkv_full, o_full
            if c.num_experts > 0:
                # Mixtral-style MoE: fused gate|up per expert + down, router.
                # TP shards WITHIN each expert (Megatron column gate|up / row
                # down); the router is replicated, and since every rank sees
                # the identical hidden states, routing agrees by construction.
                layer["router"] = W(c.num_experts, c.hidden_size)
                w13_full = W(c.num_experts, 2 * c.intermediate_size, c.hidden_size)
                w2_full = W(c.num_experts, c.hidden_size, c.intermediate_size)
                if self.ep.world > 1:  # EP first: slice this rank's experts
                    elo, ehi = self.ep.local_experts(c.num_experts)
                    w13_full = w13_full[elo:ehi]
                    w2_full = w2_full[elo:ehi]
                if tpw > 1:  # then TP-shard each (local) expert
                    layer["w13"] = torch.stack([
                        shard_gateup(w13_full[e], c.intermediate_size, self.tp)
                        for e in range(w13_full.shape[0])]).contiguous()
                    layer["w2"] = torch.stack([
                        shard_rows(w2_full[e], self.tp, dim=1)
                        for e in range(w2_full.shape[0])]).contiguous()
                    del w13_full, w2_full
                else:
                    layer["w13"] = w13_full.contiguous()
                    layer["w2"] = w2_full.contiguous()
            else:
                gateup_full = W(2 * c.intermediate_size, c.hidden_size)
                down_full = W(c.hidden_size, c.intermediate_size)
                layer["gateup"] = (shard_gateup(gateup_full, c.intermediate_size, self.tp)
                                   if tpw > 1 else gateup_full)
                layer["down"] = shard_rows(down_full, self.tp, dim=1) if tpw > 1 else down_full
                del gateup_full, down_full
            self.layers.append(layer)
        self.final_norm = torch.ones(c.hidden_size, dtype=dtype, device=self.device)
        self.lm_head = self.embed if c.tie_embeddings else W(c.vocab_size, c.hidden_size)
        if self.quant in ("fp8", "mxfp8"):
            # pre-quantize every projection weight to OCP e4m3 — halves weight
            # bytes.  "fp8": one f32 scale per output row (bf16 MFMA rate);
            # "mxfp8": e8m0 scale per 32-element K block, run on the
            # block-scaled 32x32x64 MFMA (2x fp8 rate, HW-fused dequant).
            qfn = ops.quant_fp8 if self.quant == "fp8" else ops.quant_mxfp8
            dense_projs = (("qkv", "o", "gateup", "down") if c.num_experts == 0
                           else ("qkv", "o"))
            for L in self.layers:
                for name in dense_projs:
                    q, s = qfn(L[name])
                    L[name + "_q"], L[name + "_s"] = q, s
                    del L[name]
                if c.num_experts > 0:
                    # per-expert quant (router stays bf16 — tiny)
                    for name in ("w13", "w2"):
                        E, N, K = L[name].shape
                        q, s = qfn(L[name])
                        L[name + "_q"] = q.reshape(E, N, K)
                        L[name + "_s"] = (s.reshape(E, N) if self.quant == "fp8"
                                          else s.reshape(E, N, K // 32))
                        del L[name]
            self.lm_head_q, self.lm_head_s = qfn(self.lm_head)
        self.cos_sin = ops.rope_tables(c.max_position, c.head_dim, c.rope_theta).to(self.device)
        self.scale = 1.0 / math.sqrt(c.head_dim)
        # per-layout memos of plan_tensors / _down_rows (64 entries, then clear)
        self._plan_cache = {}
        self._down_rows_cache = {}
        if self.quant == "bf16" and self.device.type == "cuda":
            # the GEMM tuner times a projection on the weights of ALL layers
            # in turn (cold from HBM, as in a forward), not on one hot buffer
            self._gemm_rotations = [
                ops.register_gemm_rotation([L[name] for L in self.layers])
                for name in ("qkv", "o", "gateup", "down") if name in self.layers[0]]

    def _linear(self, x: torch.Tensor, L: dict, name: str) -> torch.Tensor:
        """Projection through bf16 MFMA or the fp8 MFMA path.  ``L`` holds
        the weight as ``name``, or ``name_q`` / ``name_s`` on a quantized
        model: a layer dict, or ``vars(self)`` for the lm_head."""
        if self.quant == "bf16":
            return ops.gemm_bt(x, L[name])
        w_q, w_s = L[name + "_q"], L[name + "_s"]
        fp8 = self.quant == "fp8"
        if x.shape[0] <= 8 and x.is_cuda and x.shape[-1] % 1024 == 0:
            # decode: quantized-weight GEMV, activations stay bf16 (no
            # per-step quant kernel, no M-pad, half the weight stream)
            return (ops.gemv_fp8w if fp8 else ops.gemv_mxfp8w)(x, w_q, w_s)
        xq, xs = (ops.quant_fp8 if fp8 else ops.quant_mxfp8)(x)
        return (ops.gemm_bt_fp8 if fp8 else ops.gemm_bt_mxfp8)(xq, xs, w_q, w_s)

    def _layers(self, hidden: torch.Tensor,
                attend: Callable[[int, dict, torch.Tensor], torch.Tensor],
                full_rows: Optional[int] = None) -> torch.Tensor:
        """The residual stream, shared by every forward path: embedded rows
        [R, H] -> final-normed hidden states [R, H].  Per layer: pre-norm,
        qkv projection, the path's attention stage, TP all-reduce, post-norm,
        FFN.  ``attend(li, L, qkv)`` does everything between the qkv and the
        o projection inclusive and returns the o projection's partial sum
        [R, H].  ``full_rows`` (prefix-packed prefill): the unpacked row
        count, from which _down_rows picks the down projection's."""
        c = self.config
        residual = None
        for li, L in enumerate(self.layers):
            if residual is None:
                residual = hidden.clone()
                h = ops.rmsnorm(hidden, L["input_norm"], c.rms_eps)
            else:
                h = ops.fused_add_rmsnorm(hidden, residual, L["input_norm"], c.rms_eps)
            qkv = self._linear(h, L, "qkv")  # [R, local q+2kv]
            o = attend(li, L, qkv)
            self.tp.all_reduce_(o)  # row-parallel o_proj partial sum
            h = ops.fused_add_rmsnorm(o, residual, L["post_norm"], c.rms_eps)
            down_rows = None if full_rows is None else self._down_rows(h, L, full_rows)
            hidden = self._ffn(h, L, down_rows=down_rows)
        return ops.fused_add_rmsnorm(hidden, residual, self.final_norm, c.rms_eps)

    # ------------------------------------------------------------------
    # Prefill: tokens [B, S] -> final hidden states [B, S, H].
    # If `cache` is given, K/V of every position are appended (seqs maps
    # batch row -> cache sequence id).
    # ------------------------------------------------------------------
    def prefill(self, tokens: torch.Tensor, cache=None,
                seqs: Optional[List[int]] = None,
                real_lens: Optional[List[int]] = None) -> torch.Tensor:
        c = self.config
        B, S = tokens.shape
        T = B * S
        flat = tokens.reshape(T)
        positions = torch.arange(S, device=self.device, dtype=torch.int32).repeat(B)

        def attend(li, L, qkv):
            qs, kvs = self.local_q_size, self.local_kv_size
            # fused rope + [B,H,S,D] scatter reading the qkv slices in place
            qb, kb = ops.rope_scatter_qkv(qkv, self.cos_sin, positions,
                                          self.local_heads, self.local_kv_heads,
                                          c.head_dim, B, S)
            if cache is not None:
                vview = qkv[:, qs + kvs:].reshape(B, S, self.local_kv_heads, c.head_dim)
                kflat = kb.permute(0, 2, 1, 3).reshape(T, self.local_kv_heads, c.head_dim)
                vflat = vview.reshape(T, self.local_kv_heads, c.head_dim)
                for b in range(B):
                    n = real_lens[b] if real_lens is not None else S
                    cache.append(li, seqs[b], kflat[b * S: b * S + n],
                                 vflat[b * S: b * S + n].contiguous(),
                                 advance_len=(li == c.num_layers - 1))
            # V^T [B,Hk,D,S] straight from the qkv slice (LDS-tiled transpose)
            vt = ops.vt_from_qkv(qkv, self.local_heads, self.local_kv_heads,
                                 c.head_dim, B, S)
            if S % 128 == 0:
                ot = ops.attn_fwd_t(qb, kb, vt, self.scale)  # O^T [B,Hq_local,D,S]
                if self.quant == "bf16":
                    # o_proj directly off the O^T view: hipBLASLt takes the
                    # transposed A natively — no [T, qsize] copy materialized
                    return ops.gemm_bt_heads_t(ot.reshape(B, self.local_q_size, S), L["o"])
                attn = ot.permute(0, 3, 1, 2).reshape(T, self.local_q_size).contiguous()
            else:  # v1 kernel path for 64-granular sequences
                ab = ops.attn_fwd(qb, kb, None, self.scale, vt=vt)
                attn = ab.transpose(1, 2).reshape(T, self.local_q_size).contiguous()
            return self._linear(attn, L, "o")

        h = self._layers(self.embed[flat.long()], attend)  # [T, H]
        return h.reshape(B, S, c.hidden_size)

    # ------------------------------------------------------------------
    # Prefix-packed prefill: tokens [B, S] + plan -> final hidden states of
    # the Tp PACKED rows [Tp, H] (engine/prefix_plan.py).  A token prefix
    # shared by consecutive rows is computed once, in the group leader's
    # rows; everything row-wise (GEMMs, norms, SwiGLU, TP all-reduces) runs
    # on Tp rows instead of B*S.  Only rope_scatter, the V^T transpose and
    # the attention epilogue know the mapping: Q/K/V^T are expanded to the
    # ordinary [B, H, S, D] layouts (prefix broadcast to every member) and
    # attention writes straight into one packed row-major O [Tp, Hq*D].
    # ------------------------------------------------------------------
    def plan_tensors(self, plan):
        """Device copies of a plan (skip, base, owner int32 [B]; positions
        int32 [Tp]; flat token index int64 [Tp]), cached per layout: the
        scorer sees the same layout for every candidate of a step."""
        cache = self._plan_cache
        key = (plan.S, plan.owner, plan.skip)
        hit = cache.get(key)
        if hit is None:
            if len(cache) >= 64:
                cache.clear()
            pos = torch.cat([torch.arange(plan.skip[b], plan.S)
                             for b in range(plan.B)])
            row = torch.repeat_interleave(
                torch.arange(plan.B),
                torch.tensor([plan.S - s for s in plan.skip]))
            hit = tuple(t.to(self.device) for t in (
                torch.tensor(plan.skip, dtype=torch.int32),
                torch.tensor(plan.base, dtype=torch.int32),
                torch.tensor(plan.owner, dtype=torch.int32),
                pos.to(torch.int32), row * plan.S + pos))
            cache[key] = hit
        return hit

    def prefill_packed(self, tokens: torch.Tensor, plan) -> torch.Tensor:
        c = self.config
        B, S = tokens.shape
        skip, base, owner, positions, flat_idx = self.plan_tensors(plan)
        Tp = plan.Tp
        if plan.is_identity or (self.device.type == "cuda"
                                and (S % 128 != 0 or S < 256)):
            # nothing shared, or a shape the packed attention kernel does not
            # take: the unpacked path, handed back in packed-row order
            return self.prefill(tokens).reshape(B * S, -1)[flat_idx]

        def attend(li, L, qkv):
            qb, kb = ops.rope_scatter_qkv_packed(
                qkv, self.cos_sin, positions, self.local_heads,
                self.local_kv_heads, c.head_dim, B, S, skip, base, owner)
            # V stays where the qkv GEMM wrote it: the attention kernel reads
            # its rows from there (profiles/attn_v_rows.txt).  Packed
            # attention writes O row-major [Tp, Hq*D]: o_proj is a plain
            # projection (reading A as a transposed view of O^T cost the
            # GEMM 16%, profiles/gemm_lt_tuning.txt)
            attn = ops.attn_fwd_packed_qkv(
                qb, kb, qkv, self.local_heads, self.local_kv_heads,
                c.head_dim, self.scale, skip, base, owner, Tp, flat_idx)
            if self.quant == "bf16" and not attn.is_cuda:
                # CPU: the bf16 matmul the unpacked path's o_proj uses, so
                # packed and unpacked stay bit-equal there
                return torch.matmul(attn, L["o"].t())
            return self._linear(attn, L, "o")

        hidden = self.embed[tokens.reshape(B * S)[flat_idx]]  # [Tp, H]
        return self._layers(hidden, attend, full_rows=B * S)

    def _down_rows(self, h: torch.Tensor, L: dict, full_rows: int) -> Optional[int]:
        """Row count for the packed path's down projection: Tp, or the
        unpacked B*S with zero rows appended.  N = hidden is only 16 tile
        columns wide, so B*S rows are a whole number of waves over the CUs
        while Tp rows are not, and the solution the library's heuristic
        picks at Tp loses more than the rows save (605 us at M=8192 against
        901 at M=6848 for Llama-3-8B, profiles/prefix_packed_breakdown.txt).
        With the tuner on, both row counts are timed with their best
        solution and the pad is kept only where it still wins clearly with
        its zero fill counted (profiles/gemm_lt_tuning.txt); the choice is
        cached per (Tp, B*S).  Without it the pad stays, as measured."""
        Tp = h.shape[0]
        if self.quant != "bf16" or "down" not in L or full_rows <= Tp:
            return None
        cache = self._down_rows_cache
        hit = cache.get((Tp, full_rows), 0)
        if hit == 0:
            hit = full_rows
            if h.is_cuda:
                w = L["down"]
                # random data: an all-zero operand draws less power and
                # clocks higher, which would flatter both timings
                act = torch.empty(full_rows, w.shape[1], dtype=h.dtype,
                                  device=h.device).normal_()
                act[Tp:].zero_()
                t_packed = ops.gemm_lt_best_us(act[:Tp], w)
                t_full = ops.gemm_lt_best_us(act, w)
                if t_packed is not None and t_full is not None:
                    fill = ops.hip_ext().gemm_lt_fill_us(
                        act, (full_rows - Tp) * w.shape[1] * act.element_size())
                    # the pad has to win by 5%: a choice that timing noise
                    # can flip would make outputs differ between processes
                    if t_packed <= 1.05 * (t_full + fill):
                        hit = None
                elif torch.cuda.is_current_stream_capturing():
                    return full_rows  # decided outside a capture
            if len(cache) >= 64:
                cache.clear()
            cache[(Tp, full_rows)] = hit
        return hit

    def _ffn(self, h: torch.Tensor, L: dict,
             down_rows: Optional[int] = None) -> torch.Tensor:
        """``down_rows`` (dense bf16 only): run the down-projection GEMM at
        this many rows (zero rows appended to the activation, their outputs
        dropped) instead of h's row count."""
        c = self.config
        if c.num_experts == 0:
            gateup = self._linear(h, L, "gateup")
            if (self.quant == "bf16" and gateup.shape[0] == 1
                    and gateup.is_cuda
                    and os.environ.get("SENWEAVER_SWIGLU_FUSE", "0") == "1"):
                out = ops.swiglu_gemv(gateup, L["down"])
            elif self.quant == "bf16" and down_rows is not None:
                act = ops.swiglu(gateup, down_rows)
                out = self._linear(act, L, "down")[:gateup.shape[0]]
            else:
                act = ops.swiglu(gateup)
                out = self._linear(act, L, "down")
            self.tp.all_reduce_(out)  # row-parallel down_proj partial sum
            return out
        return self._moe_ffn(h, L)

    def _moe_ffn(self, h: torch.Tensor, L: dict) -> torch.Tensor:
        """Mixtral top-k routed FFN on the grouped-GEMM kernel.

        Routing/sort/combine are small tensor ops; the expert math runs as
        ONE grouped GEMM per projection (tokens sorted by expert, tile map
        built host-side so router imbalance costs no idle blocks).
        """
        c = self.config
        T = h.shape[0]
        k = c.num_experts_per_tok
        if self.quant in ("fp8", "mxfp8"):
            return self._moe_ffn_fp8(h, L)
        flat_expert, order, sorted_token, sorted_weight = self._route(h, L)
        counts = torch.bincount(flat_expert, minlength=c.num_experts)
        Tk = T * k
        if self.ep.world > 1:
            # EP: route expert-sorted tokens to their expert's owner rank,
            # grouped-GEMM the LOCAL experts, route back, combine as usual
            a_sorted = h[sorted_token]
            x_local, local_counts, meta = self.ep.dispatch(
                a_sorted, counts, c.num_experts)
            Tl = x_local.shape[0]
            a_p = self._pad128(x_local)
            seg = [0]
            for e in range(local_counts.shape[0]):
                seg.append(seg[-1] + int(local_counts[e]))
            gateup = ops.grouped_gemm_bt(a_p, L["w13"], seg)
            act = ops.swiglu(gateup[:Tl])
            down_l = ops.grouped_gemm_bt(self._pad128(act), L["w2"], seg)[:Tl]
            down = self.ep.combine(down_l, meta)
        elif h.is_cuda:
            # sync-free routing: device-side cumulative ends feed the grouped
            # GEMM directly (the per-expert int(counts[e]) reads were 8 tiny
            # D2H syncs per MoE layer, visible as copyBuffer storms in the
            # Mixtral profile and stalling the two-stream pipeline)
            offs = torch.cumsum(counts, 0).to(torch.int32)
            a_sorted = h[sorted_token]
            gateup = ops.grouped_gemm_bt(a_sorted, L["w13"], offs)[:Tk]
            act = ops.swiglu(gateup)
            down = ops.grouped_gemm_bt(act, L["w2"], offs)[:Tk]
            # fused weighted combine: inverse permutation makes each output
            # row a private k-way sum (replaces zeros + f32 index_add + cast)
            inv = torch.argsort(order).to(torch.int32).reshape(T, k)
            res = ops.hip_ext().moe_combine(down.contiguous(), inv,
                                            sorted_weight.float().contiguous())
            self.tp.all_reduce_(res)
            return res
        else:
            seg_starts = [0]
            for e in range(c.num_experts):
                seg_starts.append(seg_starts[-1] + int(counts[e]))
            a_sorted = self._pad128(h[sorted_token])
            gateup = ops.grouped_gemm_bt(a_sorted, L["w13"], seg_starts)
            act = ops.swiglu(gateup[:Tk])
            down = ops.grouped_gemm_bt(self._pad128(act), L["w2"], seg_starts)[:Tk]
        res = self._combine_f32(h, down, sorted_token, sorted_weight)
        self.tp.all_reduce_(res)  # row-parallel w2 partial sum (TP, TP x EP)
        return res

    def _route(self, h: torch.Tensor, L: dict):
        """Top-k routing of h [T, H], shared by both routed FFNs.  Returns
        (flat_expert [T*k] in token order, order: its stable argsort,
        sorted_token / sorted_weight [T*k]: token row and renormalised f32
        router weight of every slot in expert-sorted order)."""
        T = h.shape[0]
        k = self.config.num_experts_per_tok
        # router is [E=8, H]: far below the MFMA tile (N=8) — a plain skinny
        # library matmul, not a hot op
        router_logits = h @ L["router"].t()  # [T, E]
        probs = torch.softmax(router_logits.float(), dim=-1)
        topw, topi = probs.topk(k, dim=-1)           # [T, k]
        topw = topw / topw.sum(dim=-1, keepdim=True)  # renormalize (Mixtral)
        flat_expert = topi.reshape(-1)                # [T*k]
        flat_token = torch.arange(T, device=h.device).repeat_interleave(k)
        order = torch.argsort(flat_expert, stable=True)
        return flat_expert, order, flat_token[order], topw.reshape(-1)[order]

    @staticmethod
    def _pad128(x: torch.Tensor) -> torch.Tensor:
        """x [R, K] copied into a zero buffer of R + 128 rows: last-tile
        overread margin for the grouped kernel."""
        R = x.shape[0]
        p = torch.zeros(R + 128, x.shape[1], dtype=x.dtype, device=x.device)
        p[:R] = x
        return p

    @staticmethod
    def _combine_f32(h: torch.Tensor, down: torch.Tensor, sorted_token: torch.Tensor,
                     sorted_weight: torch.Tensor) -> torch.Tensor:
        """Weighted combine of the expert-sorted slot outputs ``down`` back
        into token rows where the fused moe_combine kernel does not run (EP,
        CPU): f32 zeros + index_add_, cast to h's dtype."""
        out = torch.zeros(h.shape, dtype=torch.float32, device=h.device)
        out.index_add_(0, sorted_token, down.float() * sorted_weight.unsqueeze(1))
        return out.to(h.dtype)

    def _moe_ffn_fp8(self, h: torch.Tensor, L: dict) -> torch.Tensor:
        """fp8 routed FFN: expert-sorted tokens in 16-ALIGNED padded segments
        (hipBLASLt fp8 alignment), rowwise-quantized activations, one fp8
        GEMM per non-empty expert (ops.grouped_gemm_bt_fp8).  Pad rows are
        zero -> quantize to zero -> contribute nothing."""
        c = self.config
        T = h.shape[0]
        k = c.num_experts_per_tok
        flat_expert, order, sorted_token, sorted_weight = self._route(h, L)
        sorted_expert = flat_expert[order]
        # one D2H transfer for all expert counts (16-aligned padding needs
        # host-side sizes; the bf16 path is fully sync-free)
        counts = torch.bincount(flat_expert, minlength=c.num_experts).cpu().tolist()
        seg_starts, pad_starts = [0], [0]
        for n in counts:
            seg_starts.append(seg_starts[-1] + n)
            pad_starts.append(pad_starts[-1] + ((n + 15) // 16) * 16)
        Tk = T * k
        dev = h.device
        seg_t = torch.tensor(seg_starts[:-1], device=dev)
        pad_t = torch.tensor(pad_starts[:-1], device=dev)
        # destination row of each sorted token inside its padded segment
        dest = pad_t[sorted_expert] + (torch.arange(Tk, device=dev) - seg_t[sorted_expert])
        a_pad = torch.zeros(pad_starts[-1], c.hidden_size, dtype=h.dtype, device=dev)
        a_pad[dest] = h[sorted_token]
        qfn = ops.quant_fp8 if self.quant == "fp8" else ops.quant_mxfp8
        gfn = (ops.grouped_gemm_bt_fp8 if self.quant == "fp8"
               else ops.grouped_gemm_bt_mxfp8)
        aq, a_s = qfn(a_pad)
        gateup = gfn(aq, a_s, L["w13_q"], L["w13_s"], pad_starts)
        act = ops.swiglu(gateup)
        aq2, as2 = qfn(act)
        down = gfn(aq2, as2, L["w2_q"], L["w2_s"], pad_starts)
        if h.is_cuda:
            # fused weighted combine over the PADDED layout (see _moe_ffn)
            inv_pad = dest[torch.argsort(order)].to(torch.int32).reshape(T, k)
            w_pad = torch.zeros(pad_starts[-1], dtype=torch.float32, device=dev)
            w_pad[dest] = sorted_weight.float()
            res = ops.hip_ext().moe_combine(down.contiguous(), inv_pad, w_pad)
        else:
            res = self._combine_f32(h, down[dest], sorted_token, sorted_weight)
        self.tp.all_reduce_(res)  # row-parallel down partial sum (TP)
        return res

    # ------------------------------------------------------------------
    # Decode: one new token per sequence.  tokens [B], positions [B].
    # ------------------------------------------------------------------
    def decode_step_tensors(self, tokens: torch.Tensor, pos32: torch.Tensor,
                            kcaches, vcaches, slot: torch.Tensor,
                            bt: torch.Tensor, ctx: torch.Tensor) -> torch.Tensor:
        """Graph-capturable decode step: every input is a device tensor with a
        stable address (contents may change between replays); no host reads,
        no allocations outside the caching allocator, no cache bookkeeping.

        tokens/pos32/slot: [B]; bt: [B, max_pages] int32; ctx: [B] int32.
        kcaches/vcaches: per-layer [P, 16, Hk_local, D] cache tensors.
        """
        c = self.config
        B = tokens.shape[0]

        def attend(li, L, qkv):
            P = kcaches[li].shape[0]
            # fused slice+rope+cache-append (one kernel instead of six)
            q = ops.rope_kv_append(
                qkv, self.cos_sin, pos32, slot,
                kcaches[li].view(P * 16, self.local_kv_heads, c.head_dim),
                vcaches[li].view(P * 16, self.local_kv_heads, c.head_dim),
                self.local_heads, self.local_kv_heads, c.head_dim)
            attn = ops.paged_decode_attn(q, kcaches[li], vcaches[li], bt, ctx, self.scale)
            return self._linear(attn.reshape(B, self.local_q_size), L, "o")

        # fused add+norm+GEMV path: bf16 dense decode with GEMV-eligible
        # shapes (one kernel replaces fused_add_rmsnorm + gemv per norm)
        # add+norm+GEMV fusion measured SLOWER (206 vs 218 tok/s same box):
        # every GEMV wave re-reads x/res/normw rows from L2 (3 rows instead
        # of 1), outweighing the two saved ~5us launches per layer.  Kept
        # behind the env switch as a logged A/B (profiles/r01_pmc_summary).
        fuse_ng = (self.quant == "bf16" and B <= 16
                   and os.environ.get("SENWEAVER_DECODE_NORMFUSE", "0") == "1"
                   and c.hidden_size % 512 == 0
                   and (self.local_q_size + 2 * self.local_kv_size) % 4 == 0
                   and 2 * self.local_inter % 4 == 0)
        layers = self._layers_normfuse if fuse_ng else self._layers
        return layers(self.embed[tokens], attend)

    def _layers_normfuse(self, hidden: torch.Tensor, attend) -> torch.Tensor:
        """EXPERIMENT (SENWEAVER_DECODE_NORMFUSE=1, decode_step_tensors only):
        _layers with gemv_norm_bt in place of norm + GEMV before the qkv and
        the dense gate|up projection.  The fusion crosses the seams of the
        shared loop, hence this copy of it."""
        c = self.config
        residual = None
        for li, L in enumerate(self.layers):
            qkv, residual = ops.gemv_norm_bt(hidden, residual, L["input_norm"],
                                             L["qkv"], c.rms_eps)
            o = attend(li, L, qkv)
            self.tp.all_reduce_(o)
            if c.num_experts == 0:
                gateup, residual = ops.gemv_norm_bt(o, residual, L["post_norm"],
                                                    L["gateup"], c.rms_eps)
                act = ops.swiglu(gateup)
                hidden = self._linear(act, L, "down")
                self.tp.all_reduce_(hidden)
            else:
                h = ops.fused_add_rmsnorm(o, residual, L["post_norm"], c.rms_eps)
                hidden = self._ffn(h, L)
        return ops.fused_add_rmsnorm(hidden, residual, self.final_norm, c.rms_eps)

    def decode_step(self, tokens: torch.Tensor, positions: torch.Tensor,
                    cache, seqs: List[int]) -> torch.Tensor:
        c = self.config
        B = tokens.shape[0]
        hidden = self.embed[tokens.long()]
        pos32 = positions.to(torch.int32)
        # context length for this token, captured before any append
        ctx_vals = [cache.seq_lens[s] + 1 for s in seqs]
        bt = ctx = None

        def attend(li, L, qkv):
            nonlocal bt, ctx
            qs, kvs = self.local_q_size, self.local_kv_size
            q = qkv[:, :qs].reshape(B, self.local_heads, c.head_dim).contiguous()
            k = qkv[:, qs: qs + kvs].reshape(B, self.local_kv_heads, c.head_dim).contiguous()
            v = qkv[:, qs + kvs:].reshape(B, self.local_kv_heads, c.head_dim).contiguous()
            ops.rope_inplace(q, k, self.cos_sin, pos32)
            for b in range(B):
                cache.append(li, seqs[b], k[b: b + 1], v[b: b + 1],
                             advance_len=(li == c.num_layers - 1))
            if li == 0:
                # block table / context lengths are layer-invariant for this
                # token (context = pre-append len + 1): build them once
                bt = cache.block_table_tensor(seqs)
                ctx = torch.tensor(ctx_vals, dtype=torch.int32, device=self.device)
            attn = ops.paged_decode_attn(q, cache.k[li], cache.v[li], bt, ctx, self.scale)
            return self._linear(attn.reshape(B, self.local_q_size), L, "o")

        return self._layers(hidden, attend)  # [B, hidden]

    # ------------------------------------------------------------------
    # Extend: append new_lens[b] tokens to sequences that already hold
    # cache.seq_lens[seq] positions.  tokens [B, Sq] (rows padded to Sq)
    # -> final hidden states [B, Sq, H]; pad rows carry no meaning.
    # ------------------------------------------------------------------
    def prefill_extend(self, tokens: torch.Tensor, cache, seqs: List[int],
                       new_lens: List[int]) -> torch.Tensor:
        """Prefill of a suffix against the paged cache: the new tokens'
        K/V go straight into their cache slots (rope_kv_append, real rows
        only: a pad row writes no slot and needs no rope position), then
        paged_prefill_attn reads history and new keys alike through the
        block table.  seq_lens advance once, after the last layer."""
        c = self.config
        B, Sq = tokens.shape
        assert len(seqs) == B and len(new_lens) == B
        starts = [cache.seq_lens[s] for s in seqs]
        for b in range(B):
            if not 1 <= new_lens[b] <= Sq:
                raise ValueError(f"prefill_extend: new_lens[{b}]={new_lens[b]} "
                                 f"outside [1, {Sq}]")
            if starts[b] + new_lens[b] > c.max_position:
                raise ValueError("prefill_extend: past the rope table")
            cache._ensure_capacity(seqs[b], starts[b] + new_lens[b])
        dev = self.device
        pos32 = torch.cat([torch.arange(starts[b], starts[b] + new_lens[b],
                                        dtype=torch.int32) for b in range(B)]).to(dev)
        slot = torch.cat([cache.slot_ids(seqs[b], starts[b], new_lens[b])
                          for b in range(B)]).to(torch.int32)
        # flat rows of the real tokens; None when there is no pad row
        real_idx = None
        if any(n != Sq for n in new_lens):
            real_idx = torch.cat([torch.arange(b * Sq, b * Sq + new_lens[b])
                                  for b in range(B)]).to(dev)
        bt = cache.block_table_tensor(seqs)
        ctx = torch.tensor([starts[b] + new_lens[b] for b in range(B)],
                           dtype=torch.int32, device=dev)
        qlen = torch.tensor(new_lens, dtype=torch.int32, device=dev)

        Hq, Hk, D = self.local_heads, self.local_kv_heads, c.head_dim

        def attend(li, L, qkv):
            P = cache.k[li].shape[0]
            q_real = ops.rope_kv_append(
                qkv if real_idx is None else qkv[real_idx],
                self.cos_sin, pos32, slot,
                cache.k[li].view(P * 16, Hk, D), cache.v[li].view(P * 16, Hk, D),
                Hq, Hk, D)
            if real_idx is None:
                q = q_real.reshape(B, Sq, Hq, D)
            else:
                q = q_real.new_zeros(B * Sq, Hq, D)
                q[real_idx] = q_real
                q = q.reshape(B, Sq, Hq, D)
            attn = ops.paged_prefill_attn(q, cache.k[li], cache.v[li], bt, ctx,
                                          qlen, self.scale)
            return self._linear(attn.reshape(B * Sq, self.local_q_size), L, "o")

        h = self._layers(self.embed[tokens.reshape(B * Sq).long()], attend)
        for b in range(B):
            cache.seq_lens[seqs[b]] = starts[b] + new_lens[b]
        return h.reshape(B, Sq, c.hidden_size)

    def logits(self, hidden: torch.Tensor) -> torch.Tensor:
        """hidden [*, H] -> logits [*, vocab] through the lm_head GEMM."""
        return self._linear(hidden.reshape(-1, self.config.hidden_size), vars(self), "lm_head")
