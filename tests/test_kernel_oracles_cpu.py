"""CPU checks of the decode-kernel, prefill-attention, quantized GEMM /
quantizer / MoE, dense bf16 GEMM and elementwise oracles
(tests/kernel_oracles.py).

Three things are established without a GPU:
1. each fp64 oracle agrees with the existing fp32 reference in
   senweaver_amd.ops.reference on random data;
2. every input generator satisfies the condition its GPU test relies on
   (score gap, integer-sum magnitude, power-of-two scales, exact
   representability of the bit-exact expectations);
3. the ops.* CPU fallbacks pass the same edge cases the GPU kernels get;
4. every check rejects operators that are wrong in the way it is meant to
   catch (and accepts a legitimately different one).
"""

import math

import pytest
import torch

import kernel_oracles as ko
from senweaver_amd import ops
from senweaver_amd.ops import reference as ref


@pytest.fixture
def gen():
    return torch.Generator().manual_seed(1234)


CPU = torch.device("cpu")


# ---------------- 1. oracles vs the fp32 references ----------------
def test_gemv_ref64_matches_fp32_reference(gen):
    x, w = ko.rand_bf16(gen, 5, 1536), ko.rand_bf16(gen, 12, 1536)
    r64 = ko.gemv_ref64(x, w.double())
    r32 = x.float() @ w.float().t()
    torch.testing.assert_close(r64.float(), r32, rtol=1e-5, atol=1e-3)
    # and the committed reference's bf16 result is the rounding of the oracle
    # up to the fp32 summation error
    ko.assert_within(ref.gemm_bt_ref(x, w), r64,
                     ko.gemv_bound(r64, ko.gemv_abs_dot(x, w.double()), 1536))


def test_dequant_oracles_match_fp32_reference(gen):
    N, K = 12, 1024
    (q, s), w64 = ko.make_weights("fp8", gen, N, K, "random_scale")
    wf = q.view(torch.float8_e4m3fn).float() * s.unsqueeze(1)
    torch.testing.assert_close(w64.float(), wf, rtol=1e-6, atol=0)
    (q, s), w64 = ko.make_weights("mx", gen, N, K, "random")
    f = q.view(torch.float8_e4m3fn).float().view(N, K // 32, 32)
    wf = (f * torch.exp2(s.float() - 127).unsqueeze(-1)).reshape(N, K)
    assert torch.equal(w64.float(), wf)
    # against the committed mx GEMM reference with an identity-like activation
    a_q = torch.zeros(1, K, dtype=torch.uint8)
    a_q[0, 40] = torch.tensor(1.0).to(torch.float8_e4m3fn).view(torch.uint8)
    a_s = torch.full((1, K // 32), 127, dtype=torch.uint8)
    got = ref.gemm_bt_mxfp8_ref(a_q, a_s, q, s)
    ko.assert_bits_equal(got, ko.exact_bf16(w64[:, 40].unsqueeze(0)))


def test_gemv_norm_ref64_matches_reference_composition(gen):
    M, N, K, eps = 3, 12, 1536, 1e-5
    x, res = ko.rand_bf16(gen, M, K), ko.rand_bf16(gen, M, K)
    normw, b = ko.rand_bf16(gen, K), ko.rand_bf16(gen, N, K)
    c64, res_out, absdot = ko.gemv_norm_ref64(x, res, normw, b, eps)
    # fp32 evaluation of the same (unrounded-t) definition
    t = x.float() + res.float()
    c32 = ((t * normw.float()) @ b.float().t()) * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + eps)
    torch.testing.assert_close(c64.float(), c32, rtol=1e-4, atol=1e-3)
    # the committed composition rounds t and y to bf16: it agrees to bf16 accuracy
    y, r = ref.fused_add_rmsnorm_ref(x, res, normw, eps)
    ko.assert_bits_equal(res_out, r)
    assert ko.rel_fro(ref.gemm_bt_ref(y, b), c64) <= 2.0 ** -7
    assert bool((absdot >= c64.abs()).all())
    c64n, ro, _ = ko.gemv_norm_ref64(x, None, normw, b, eps)
    ko.assert_bits_equal(ro, x)
    assert ko.rel_fro(ref.gemm_bt_ref(ref.rmsnorm_ref(x, normw, eps), b), c64n) <= 2.0 ** -7


def test_swiglu_ref64_matches_fp32_reference(gen):
    gu = ko.rand_bf16(gen, 2, 2048)
    a64 = ko.swiglu_ref64(gu)
    ko.assert_within(ref.swiglu_ref(gu), a64, 2.0 ** -8 * a64.abs() + 1e-30)


def test_paged_attn_ref64_matches_fp32_reference(gen):
    case = ko.make_paged_case(gen, [1, 37, 200], 8, 2)
    r64 = ko.paged_decode_attn_ref64(**case)
    r32 = ref.paged_decode_attn_ref(**case)
    ko.assert_within(r32, r64, torch.tensor(ko.attn_bound(case["vcache"])))


def test_rope_ref64_matches_fp32_reference(gen):
    x = ko.rand_bf16(gen, 6, 5, 64)
    cs = ops.rope_tables(100, 64)
    pos = torch.tensor([0, 1, 17, 99, 50, 0], dtype=torch.int32)
    r64, bound = ko.rope_ref64(x, cs, pos)
    ko.assert_within(ref.rope_ref(x, cs, pos), r64, bound)
    # position 0 is the identity
    assert torch.equal(r64[0], x[0].double()) and torch.equal(r64[5], x[5].double())


def test_target_logprob_ref64_matches_fp32_reference(gen):
    logits = ko.rand_bf16(gen, 4, 1000)
    tgt = torch.tensor([0, 999, 5, 500], dtype=torch.int32)
    torch.testing.assert_close(ko.target_logprob_ref64(logits, tgt).float(),
                               ref.target_logprob_ref(logits, tgt), rtol=1e-5, atol=1e-5)


# ---------------- 2. generator premises ----------------
def test_probe_columns_cover_boundaries():
    assert ko.probe_columns(512) == [0, 7, 8, 15, 16, 511]
    p = ko.probe_columns(14336)
    for c in (0, 7, 8, 15, 16, 511, 512, 1023, 1024, 3071, 3072, 13312, 13823, 13824, 14335):
        assert c in p
    for K in (512, 1024, 1536, 3072, 4096, 5120, 14336):
        P = ko.probe_columns(K)
        assert all(0 <= c < K for c in P) and K - 1 in P
        for M in (1, 2, 3, 4, 5, 8, 9, 16):
            calls = ko.onehot_calls(M, K)
            assert all(len(c) == M for c in calls)
            assert {k for c in calls for k in c} == set(P)  # every probe at every M
    x = ko.onehot_x([3, 0], 16)
    assert x.sum() == 2 and x[0, 3] == 1 and x[1, 0] == 1


@pytest.mark.parametrize("kind", ["bf16", "fp8", "mx"])
def test_onehot_expectations_are_exact_bf16(gen, kind):
    """W[:, k] (dequantized with power-of-two scales) is a bf16 value, is
    never +-0 / non-finite, and W is not symmetric."""
    (wargs, w64) = ko.make_weights(kind, gen, 24, 1024, "random")
    assert torch.equal(w64.to(torch.bfloat16).double(), w64)
    assert bool(torch.isfinite(w64).all()) and bool((w64 != 0).all())
    assert not torch.equal(w64[:, :24], w64[:, :24].t())
    if kind == "fp8":
        assert bool(ko.is_pow2(wargs[1]).all())
    if kind == "mx":
        assert wargs[1].dtype == torch.uint8 and wargs[1].shape == (24, 32)
        assert bool(ko.is_pow2(torch.exp2(wargs[1].double() - 127)).all())


@pytest.mark.parametrize("kind,K", [("bf16", 14336), ("bf16", 15360), ("fp8", 4096), ("mx", 4096),
                                    ("qgemm-fp8", 640), ("qgemm-mx", 640), ("grouped", 192),
                                    ("combine", 2056)])
def test_integer_sums_stay_exact_in_fp32(gen, kind, K):
    """sum |x||w| (an upper bound on every partial sum in any order), in
    units of the smallest scale 2^-3, stays below 2^24.  The tiled quantized
    GEMM, grouped GEMM and combine generators: the same in their own units
    (unscaled integers / 2^-4 / integers / 2^-3)."""
    if kind.startswith("qgemm"):
        q = kind[len("qgemm-"):]
        args, a64, b64 = ko.make_qgemm_case(q, "int", gen, 130, 140, K)
        assert ko.qgemm_int_premise(q, args, a64, b64) < 2 ** 24
        unit = 1 if q == "fp8" else 16      # fp8: the accumulator is unscaled
        for t in ((ko.e4m3_to_f64(args[0]), ko.e4m3_to_f64(args[2])) if q == "fp8"
                  else (a64, b64)):
            assert float(t.abs().max()) <= (4 if q == "fp8" else 16)
        prod = a64 @ b64.t()
        assert torch.equal(prod * 64 * unit, (prod * 64 * unit).round())
        ko.exact_bf16(prod)
        s = (torch.cat([args[1], args[3]]).double() if q == "fp8"
             else torch.exp2(torch.cat([args[1], args[3]]).double() - 127))
        assert bool(ko.is_pow2(s).all())
        return
    if kind == "grouped":
        a, w, starts, ref64, absdot = ko.make_grouped_case(gen, [3, 0, 130], 128, K, "int")
        assert float(absdot.max()) < 2 ** 24 and torch.equal(ref64, ref64.round())
        ko.exact_bf16(ref64)
        return
    if kind == "combine":
        down, pos, w, ref64, absum = ko.make_combine_case(gen, 7, 3, K, "pow2")
        assert float(absum.max()) * 8 < 2 ** 24 and torch.equal(ref64 * 8, (ref64 * 8).round())
        assert bool(ko.is_pow2(w[w != 0]).all())
        ko.exact_bf16(ref64)
        return
    (wargs, w64) = ko.make_weights(kind, gen, 12, K, "int")
    x = ko.int_x(gen, 16, K)
    assert float(x.double().abs().max()) <= 2
    ad = ko.gemv_abs_dot(x, w64)
    assert float(ad.max()) * 8 < 2 ** 24
    ref64 = ko.gemv_ref64(x, w64)
    assert torch.equal(ref64 * 8, (ref64 * 8).round())       # multiples of 2^-3
    ko.exact_bf16(ref64)                                      # asserts fp32-exactness
    if kind == "bf16":
        assert float(w64.abs().max()) <= 4 and torch.equal(w64, w64.round())
    else:
        assert float(ko.e4m3_to_f64(wargs[0]).abs().max()) <= 4
        s = wargs[1].double() if kind == "fp8" else torch.exp2(wargs[1].double() - 127)
        assert bool(ko.is_pow2(s).all()) and float(s.min()) >= 2 ** -3


def test_swiglu_onehot_activation_is_exact(gen):
    gu = ko.swiglu_onehot_gateup(gen, 700, 1024)
    # fp32: 1 + exp(-32) rounds to 1, so silu(32) = 32 exactly
    assert float(torch.tensor(1.0) + torch.exp(torch.tensor(-32.0))) == 1.0
    act = ref.swiglu_ref(gu)
    exp = torch.zeros(1, 1024, dtype=torch.bfloat16)
    exp[0, 700] = 32.0
    assert torch.equal(act.float(), exp.float())


@pytest.mark.parametrize("ctx", [1, 7, 9, 16, 17, 33, 257, 1032, 2100])
def test_paged_spike_gap(gen, ctx):
    pp = ko.probe_positions(ctx)
    chunk = -(-ctx // 8)
    assert 0 in pp and ctx - 1 in pp and all(0 <= p < ctx for p in pp)
    if ctx == 2100:
        assert {chunk - 1, chunk, chunk + 127, chunk + 128} <= set(pp)
    case = ko.make_paged_case(gen, [ctx], 2, 2)
    bt = case["block_table"]
    used = bt[bt >= 0]
    assert used.numel() == -(-ctx // 16) == used.unique().numel()
    assert bt.shape[1] > used.numel() and int(bt[0, -1]) == -1
    for i, p in enumerate(pp):
        kc, gap, v_row = ko.plant_spike(case, 0, i % 2, p)
        assert gap >= 60.0
        assert not torch.equal(kc, case["kcache"])
        # the oracle itself returns V[p*] to well below half a bf16 ulp
        c2 = dict(case, kcache=kc)
        r = ko.paged_decode_attn_ref64(**c2)[0, i % 2]
        assert float((r - v_row.double()).abs().max()) < 1e-20


def test_paged_block_table_is_permuted(gen):
    case = ko.make_paged_case(gen, [1, 1032, 2100], 8, 2)
    bt = case["block_table"]
    used = bt[bt >= 0]
    assert used.unique().numel() == used.numel() == 1 + 65 + 132
    assert not torch.equal(bt[2, :132], torch.arange(132, dtype=torch.int32))
    assert int((bt[0] == -1).sum()) == bt.shape[1] - 1


# ---------------- 2b. the checks notice subtly wrong operators ----------------
def _next_bf16(t):
    """One bf16 ulp away from t (bit pattern + 1)."""
    return (t.contiguous().view(torch.int16) + 1).view(torch.bfloat16)


def test_gemv_checks_catch_wrong_kernels(gen):
    K = 1536

    def drop_last_slot(x, w):          # the K % 1024 bug: last 512 columns lost
        x = x.clone()
        x[:, K - 512:] = 0
        return ops.gemm_bt(x, w)

    def swap_lanes(x, w):              # columns 7 and 8 exchanged
        x = x.clone()
        x[:, [7, 8]] = x[:, [8, 7]]
        return ops.gemm_bt(x, w)

    def one_ulp_off(x, w):             # one output element one bf16 ulp away
        c = ops.gemm_bt(x, w)
        c[0, 0] = _next_bf16(c[0, 0])
        return c

    def last_row_stale(x, w):          # M tail row not written
        c = ops.gemm_bt(x, w)
        c[-1] = 0
        return c

    for bad in (drop_last_slot, swap_lanes, one_ulp_off, last_row_stale):
        with pytest.raises(AssertionError):
            ko.check_gemv_onehot(bad, "bf16", [1, 3], [12], K, CPU, gen)
    for bad in (drop_last_slot, one_ulp_off, last_row_stale):
        with pytest.raises(AssertionError):
            ko.check_gemv_int(bad, "bf16", [3], [12], K, CPU, gen)
    for bad in (drop_last_slot, last_row_stale):
        with pytest.raises(AssertionError):
            ko.check_gemv_random(bad, "bf16", [3], [12], K, CPU, gen)

    def drop_slot_swiglu(gu, w):
        gu = gu.clone()
        gu[:, 5120 - 512:5120] = 0      # silu(0) = 0: last 512 activations lost
        return ops.swiglu_gemv(gu, w)

    with pytest.raises(AssertionError):
        ko.check_swiglu_random(drop_slot_swiglu, [264], 5120, CPU, gen)
    with pytest.raises(AssertionError):
        ko.check_swiglu_onehot(drop_slot_swiglu, [12], 5120, CPU, gen)


def test_gemv_norm_check_catches_wrong_kernels(gen):
    def no_residual_in_norm(x, res, normw, b, eps):   # sum of squares over x only
        c, r = ops.gemv_norm_bt(x, res, normw, b, eps)
        c2, _ = ops.gemv_norm_bt(x, None, normw, b, eps)
        return c2, r

    def res_out_one_ulp_off(x, res, normw, b, eps):
        c, r = ops.gemv_norm_bt(x, res, normw, b, eps)
        r = r.clone()
        r[0, -1] = _next_bf16(r[0, -1])
        return c, r

    for bad in (no_residual_in_norm, res_out_one_ulp_off):
        with pytest.raises(AssertionError):
            ko.check_gemv_norm(bad, [3], [12], 512, CPU, gen, True, fro_tol=2.0 ** -7)


def test_paged_checks_catch_wrong_kernels(gen):
    def contiguous_table(q, kc, vc, bt, ctx, scale):   # ignores the block table
        bt = torch.arange(bt.shape[1], dtype=torch.int32).repeat(bt.shape[0], 1)
        return ops.paged_decode_attn(q, kc, vc, bt, ctx, scale)

    def drop_last_position(q, kc, vc, bt, ctx, scale):
        return ops.paged_decode_attn(q, kc, vc, bt, (ctx - 1).clamp(min=1), scale)

    def no_rescale(q, kc, vc, bt, ctx, scale):         # merge forgets one split
        o = ops.paged_decode_attn(q, kc, vc, bt, ctx, scale)
        o2 = ops.paged_decode_attn(q, kc, vc, bt, (ctx * 7 // 8).clamp(min=1), scale)
        return ((o.float() + o2.float()) / 2).to(torch.bfloat16)

    for bad in (contiguous_table, drop_last_position):
        with pytest.raises(AssertionError):
            ko.check_paged_onehot(bad, 33, CPU, gen)
    for bad in (contiguous_table, no_rescale):
        with pytest.raises(AssertionError):
            ko.check_paged_random(bad, (1, 40, 300), 8, 2, CPU, gen, "late_spike")


def test_rope_check_catches_stray_write_and_wrong_rotation(gen):
    def stray_write(qkv, cs, pos, slot, kc, vc, Hq, Hk, D):
        q = ops.rope_kv_append(qkv, cs, pos, slot, kc, vc, Hq, Hk, D)
        kc[3, Hk - 1, D - 1] = 0.0     # a slot nobody named
        return q

    def wrong_position(qkv, cs, pos, slot, kc, vc, Hq, Hk, D):
        return ops.rope_kv_append(qkv, cs, (pos + 1).clamp(max=cs.shape[0] - 1), slot,
                                  kc, vc, Hq, Hk, D)

    def last_head_skipped(qkv, cs, pos, slot, kc, vc, Hq, Hk, D):
        q = ops.rope_kv_append(qkv, cs, pos, slot, kc, vc, Hq, Hk, D)
        vc[slot.long(), Hk - 1] = ko.SENTINEL   # second y-block's tail never ran
        return q

    for bad in (stray_write, wrong_position, last_head_skipped):
        with pytest.raises(AssertionError):
            ko.check_rope_kv_append(bad, 32, 8, 128, CPU, gen, ops.rope_tables)


def test_sampling_checks_catch_wrong_kernels(gen):
    def torch_argmax(logits):          # NaN wins in torch.argmax
        return logits.float().argmax(dim=-1).to(torch.int32)

    def last_index_on_tie(logits):
        x = logits.float().flip(-1)
        x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
        return (logits.shape[-1] - 1 - x.argmax(dim=-1)).to(torch.int32)

    for bad in (torch_argmax, last_index_on_tie):
        with pytest.raises(AssertionError):
            ko.check_argmax(bad, 2056, CPU, gen)

    def nan_on_neg_inf(logits, tgt):   # the -inf - -inf combine
        x = logits.float()
        m = x[:, :8].max(dim=-1, keepdim=True).values     # first vector only
        lse = m + torch.log(torch.exp(x - m).sum(-1, keepdim=True))
        return (x - lse).gather(1, tgt.long().unsqueeze(1)).squeeze(1)

    with pytest.raises(AssertionError):
        ko.check_target_logprob(nan_on_neg_inf, 512, CPU, gen)


# ---------------- 3. ops.* CPU fallbacks on the edge cases ----------------
@pytest.mark.parametrize("kind,fn,K", [
    ("bf16", ops.gemm_bt, 512), ("bf16", ops.gemm_bt, 1536),
    ("fp8", ops.gemv_fp8w, 1024), ("mx", ops.gemv_mxfp8w, 3072)])
def test_cpu_gemv_fallbacks(gen, kind, fn, K):
    Ms = [1, 3, 5, 16] if kind == "bf16" else [1, 3, 8]
    ko.check_gemv_onehot(fn, kind, Ms, [4, 12], K, CPU, gen)
    ko.check_gemv_int(fn, kind, Ms, [4, 12], K, CPU, gen)
    ko.check_gemv_random(fn, kind, Ms, [4, 12], K, CPU, gen)
    if kind == "fp8":
        ko.check_gemv_random(fn, kind, Ms, [12], K, CPU, gen, mode="random_scale")


def test_cpu_gemv_norm_fallback(gen):
    # the fallback rounds t and y to bf16 (three bf16 roundings in all), so
    # it is held to a relative Frobenius error of 2^-7 instead of the
    # kernel's elementwise fp32 bound; res_out is still bit-equal
    for with_res in (True, False):
        ko.check_gemv_norm(ops.gemv_norm_bt, [1, 3, 16], [12], 512, CPU, gen, with_res,
                           fro_tol=2.0 ** -7)


def test_cpu_swiglu_gemv_fallback(gen):
    ko.check_swiglu_onehot(ops.swiglu_gemv, [12], 5120, CPU, gen)
    ko.check_swiglu_random(ops.swiglu_gemv, [12, 264], 5120, CPU, gen)


@pytest.mark.parametrize("ctx", [1, 7, 33, 257])
def test_cpu_paged_attn_onehot(gen, ctx):
    ko.check_paged_onehot(ops.paged_decode_attn, ctx, CPU, gen)


@pytest.mark.parametrize("mode", ["diffuse", "peaked", "late_spike"])
def test_cpu_paged_attn_random(gen, mode):
    ko.check_paged_random(ops.paged_decode_attn, (1, 40, 300), 8, 2, CPU, gen, mode)


@pytest.mark.parametrize("Hq,Hk,D", [(32, 8, 128), (4, 2, 64)])
def test_cpu_rope_fallbacks(gen, Hq, Hk, D):
    ko.check_rope_kv_append(ops.rope_kv_append, Hq, Hk, D, CPU, gen, ops.rope_tables)
    ko.check_rope_scatter(ops.rope_scatter_qkv, Hq, Hk, D, CPU, gen, ops.rope_tables,
                          B=2, S=8)


@pytest.mark.parametrize("vocab", [8, 512, 1000, 1003, 2056])
def test_cpu_argmax_fallback(gen, vocab):
    ko.check_argmax(ops.argmax_rows, vocab, CPU, gen)


@pytest.mark.parametrize("vocab", [8, 512, 1000, 2048])
def test_cpu_target_logprob_fallback(gen, vocab):
    ko.check_target_logprob(ops.target_logprob, vocab, CPU, gen)


# ==========================================================================
# Prefill attention: oracle, generator premises, CPU fallbacks and the wrong
# operators each check has to reject (test_prefill_edges_gpu.py runs the
# same checks on the HIP kernels).
# ==========================================================================
PREFILL_SEED = 20241      # the seed of test_prefill_edges_gpu.py's generator
HEAD_CONFIGS = [(1, 1, 1), (2, 4, 2), (1, 6, 2)]
ALL_POINTER_S = [64, 128, 192, 256, 320, 384, 512, 640]


@pytest.fixture
def pgen():
    return torch.Generator().manual_seed(PREFILL_SEED)


def _ops_attn_fwd(q, k, vt, s):
    return ops.attn_fwd(q, k, None, s, vt=vt).transpose(-1, -2).contiguous()


def attn_variant(mask="causal", kv_map="div", batch0=False, transposed=True,
                 p_bf16=False, tiled=None):
    """An fp64 attention operator built from the reference with one property
    switched.  mask: 'causal' | 'ge' (kv >= q hidden) | 'plus1' (kv > q+1
    hidden) | 'skip32' (the first row of every 32-row group sees its whole
    64-key tile).  kv_map: 'div' (h // rep) | 'mod' (h % Hk).  p_bf16: P
    rounded to bf16 AND l summed from the rounded values.  tiled: None, or
    64-key online softmax with the 8-nat defer rule, 'ok' or 'bug' (deferred
    tiles add exp(s - m - 8) to O while l sums exp(s - m))."""
    def fn(q, k, vt, scale):
        q, k, v = q.cpu(), k.cpu(), vt.cpu().transpose(-1, -2)
        B, H, S, D = q.shape
        Hk = k.shape[1]
        i, j = torch.arange(S).view(S, 1), torch.arange(S).view(1, S)
        hidden = {"causal": j > i, "ge": j >= i, "plus1": j > i + 1,
                  "skip32": (j > i) & ~((i % 32 == 0) & (j < 64 * (i // 64) + 64))}[mask]
        kvh = torch.arange(H) // (H // Hk) if kv_map == "div" else torch.arange(H) % Hk
        out = torch.empty(B, H, S, D, dtype=torch.float64)
        for b in range(B):
            bb = 0 if batch0 else b
            s = (q[b].double() @ k[bb, kvh].double().transpose(-1, -2)) * scale
            s = s.masked_fill(hidden, float("-inf"))
            vv = v[bb, kvh].double()
            if tiled is None:
                p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
                if p_bf16:
                    p = p.to(ko.BF16).double()
                out[b] = (p @ vv) / p.sum(dim=-1, keepdim=True)
                continue
            m = torch.full((H, S, 1), float("-inf"), dtype=torch.float64)
            l = torch.zeros(H, S, 1, dtype=torch.float64)
            o = torch.zeros(H, S, D, dtype=torch.float64)
            for t0 in range(0, S, 64):
                st = s[:, :, t0:t0 + 64]
                tm = st.max(dim=-1, keepdim=True).values
                defer = (tm - m) <= ko.DEFER_THRESHOLD      # NaN / +inf: False
                m_new = torch.where(defer, m, torch.maximum(m, tm))
                alpha = torch.where(m == float("-inf"), torch.zeros_like(m),
                                    torch.exp(m - m_new))
                p = torch.exp(st - m_new)
                l = l * alpha + p.sum(dim=-1, keepdim=True)
                if tiled == "bug":
                    p = torch.where(defer, p * math.exp(-8.0), p)
                o = o * alpha + p @ vv[:, t0:t0 + 64]
                m = m_new
            out[b] = o / l
        o16 = out.to(ko.BF16)
        return o16.transpose(-1, -2).contiguous() if transposed else o16
    return fn


# ---------------- oracle agreement ----------------
def test_attn_prefill_ref64_matches_fp32_reference(gen):
    for B, H, Hk, S in [(2, 4, 2, 192), (1, 6, 2, 128)]:
        c = ko.make_prefill_case(gen, "peaked", B, H, Hk, S)
        r64 = ko.attn_prefill_ref64(c["q"], c["k"], c["v"], c["scale"])
        r32 = ref.attn_fwd_ref(c["q"], c["k"], c["v"], c["scale"], causal=True)
        # the fp32 reference rounds its output to bf16 and nothing else
        ko.assert_within(r32, r64, ko.U_BF16_OUT * r64.abs() + 1e-5)
        # row 0 sees one key
        kvh = ko.kv_head_of(H, Hk)
        assert torch.equal(r64[:, :, 0], c["v"][:, kvh][:, :, 0].double())
    # and the tiled fp64 formulation (with defers) is the same function
    c = ko.make_prefill_case(gen, "stair+3", 1, 4, 2, 384)
    r64 = ko.attn_prefill_ref64(c["q"], c["k"], c["v"], c["scale"])
    got = attn_variant(tiled="ok")(c["q"], c["k"], c["vt"], c["scale"])
    ko.assert_within(got.transpose(-1, -2), r64, ko.U_BF16_OUT * r64.abs() + 1e-12)


# ---------------- generator premises ----------------
def test_pointer_targets_hit_the_edges():
    g = torch.Generator().manual_seed(0)
    i = torch.arange(320)
    assert torch.equal(ko.pointer_targets("diag", 320, g), i)
    assert int(ko.pointer_targets("first", 320, g).max()) == 0
    t = ko.pointer_targets("tile_first", 320, g)
    assert [int(t[x]) for x in (0, 63, 64, 127, 319)] == [0, 0, 64, 64, 256]
    t = ko.pointer_targets("tile_prev_last", 320, g)
    assert [int(t[x]) for x in (0, 63, 64, 127, 128, 319)] == [0, 0, 63, 63, 127, 255]
    t = ko.pointer_targets("wave_prev_last", 320, g)   # kv0 + 63 == q0 - 1 + 32 k
    assert [int(t[x]) for x in (0, 31, 32, 63, 64, 96, 319)] == [0, 0, 31, 31, 63, 95, 287]
    t = ko.pointer_targets("random", 320, g)
    assert bool((t <= i).all()) and int(t[0]) == 0 and len(set(t.tolist())) > 100


@pytest.mark.parametrize("S", ALL_POINTER_S)
def test_pointer_premises_every_row(pgen, S):
    """Gap >= 60 nats for EVERY row (pointer_min_gap takes the minimum over
    all rows, the other keys over the whole sequence), V clamped, integer
    scores, distinct V per (batch, kv head) — for every map and head
    configuration, drawn as the GPU test draws them."""
    for tmap in ko.POINTER_MAPS:
        g = torch.Generator().manual_seed(PREFILL_SEED)
        for B, H, Hk in HEAD_CONFIGS:
            c = ko.make_pointer_case(g, B, H, Hk, S, tmap)
            gap = ko.pointer_min_gap(c["q"], c["k"], c["t"], c["scale"])
            assert gap >= ko.POINTER_MIN_GAP, (S, tmap, gap)
            assert float(c["v"].abs().min()) >= ko.V_FLOOR
            assert set(c["k"].unique().tolist()) == {-1.0, 1.0}
            assert set(c["q"].unique().tolist()) == {-16.0, 16.0}
            kvh = ko.kv_head_of(H, Hk)
            tgt = (c["q"].double() * c["k"][:, kvh][:, :, c["t"]].double()).sum(-1)
            assert bool((tgt == 16.0 * 128).all())          # 181.02 nats
            assert c["expected"].shape == (B, H, S, ko.PREFILL_D)


def test_pointer_premises_dispatch_shapes(pgen):
    for B, H, Hk in [(1, 512, 512), (1, 511, 511), (2, 256, 64)]:
        for tmap in ("diag", "random"):
            g = torch.Generator().manual_seed(PREFILL_SEED)
            c = ko.make_pointer_case(g, B, H, Hk, 256, tmap)
            assert ko.pointer_min_gap(c["q"], c["k"], c["t"], c["scale"]) >= ko.POINTER_MIN_GAP


def test_clamp_v():
    v = torch.tensor([0.0, -0.0, 2.0 ** -7, -(2.0 ** -7), 2.0 ** -6, -3.0, 0.5]).to(ko.BF16)
    got = ko.clamp_v(v)
    assert got.tolist() == [2.0 ** -6, 2.0 ** -6, 2.0 ** -6, -(2.0 ** -6), 2.0 ** -6, -3.0, 0.5]


@pytest.mark.parametrize("S", ALL_POINTER_S)
def test_decoy_premises(pgen, S):
    """Run on the exact oracle: the check asserts its own premises (decoy
    lead >= 60 nats, separation from V[i+1] > 4 bounds for every row >= 1,
    score range) before it looks at the operator's output."""
    ratio = ko.check_future_decoy(attn_variant(), 2, 4, 2, S, CPU, pgen)
    assert ratio <= 1.0   # bf16 output rounding only: half an ulp <= 2^-8 |o|


@pytest.mark.parametrize("S", [192, 320, 384, 640])
@pytest.mark.parametrize("mode", ko.PREFILL_MODES)
def test_random_case_premises(pgen, mode, S):
    c = ko.make_prefill_case(pgen, mode, 1, 4, 2, S)
    assert ko.max_abs_score_log2(c["q"], c["k"], c["scale"]) <= ko.SCORE_LOG2_MAX
    if mode.startswith("stair"):
        ko.assert_stair_premises(c["q"], c["k"], c["scale"], mode)


def test_defer_pattern_regimes():
    step = lambda d, n: torch.arange(n, dtype=torch.float64) * d
    assert ko.defer_pattern(step(3.0, 7)) == "RDDRDDR"
    assert ko.defer_pattern(step(7.0, 6)) == "RDRDRD"
    assert ko.defer_pattern(step(9.0, 5)) == "RRRRR"
    assert ko.defer_pattern(step(-7.0, 5)) == "RDDDD"
    assert ko.defer_pattern(torch.tensor([0.0, 8.0, 8.5, 16.5])) == "RDRD"


# ---------------- CPU fallbacks, smallest S of each list ----------------
@pytest.mark.parametrize("tmap", ko.POINTER_MAPS)
@pytest.mark.parametrize("S", [64, 128])
def test_cpu_prefill_pointer(pgen, S, tmap):
    for B, H, Hk in HEAD_CONFIGS:
        ko.check_pointer(ops.attn_fwd_t, B, H, Hk, S, tmap, CPU, pgen)
        ko.check_pointer(_ops_attn_fwd, B, H, Hk, S, tmap, CPU, pgen)


@pytest.mark.parametrize("S", [64, 128])
def test_cpu_prefill_future_decoy(pgen, S):
    ko.check_future_decoy(ops.attn_fwd_t, 2, 4, 2, S, CPU, pgen)
    ko.check_future_decoy(_ops_attn_fwd, 2, 4, 2, S, CPU, pgen)


@pytest.mark.parametrize("mode", ko.PREFILL_MODES)
@pytest.mark.parametrize("S", [192, 384])
def test_cpu_prefill_vs_fp64(pgen, S, mode):
    ko.check_prefill_random(ops.attn_fwd_t, mode, 1, 4, 2, S, CPU, pgen)


def test_cpu_prefill_dispatch_shapes_and_views(pgen):
    """The public ops at a dispatch shape and on permuted [B,S,H,D] views
    (on the CPU both run the fp32 reference)."""
    def bshd_view(t):
        view = t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
        assert not view.is_contiguous()
        return view

    ko.check_pointer(ops.attn_fwd_t, 2, 256, 64, 256, "random", CPU, pgen)
    for fn, S in ((ops.attn_fwd_t, 256), (_ops_attn_fwd, 192)):
        for tmap in ("diag", "random"):
            ko.check_pointer(fn, 2, 4, 2, S, tmap, CPU, pgen, prep=bshd_view)


@pytest.mark.parametrize("S", [1, 7, 8, 31, 33, 100])
def test_cpu_vt_from_qkv(pgen, S):
    for D in (64, 128):
        for Hq, Hk in [(1, 1), (4, 2), (6, 2)]:
            for B in (1, 2):
                ko.check_vt_from_qkv(ops.vt_from_qkv, B, S, Hq, Hk, D, CPU, pgen)
    ko.check_vt_from_qkv(ops.vt_from_qkv, 2, S, 4, 2, 128, CPU, pgen, extra_cols=8)

    def drops_last_column(qkv, Hq, Hk, D, B, S_):
        vt = ops.vt_from_qkv(qkv, Hq, Hk, D, B, S_).clone()
        vt[..., S_ - 1] = 0
        return vt

    with pytest.raises(AssertionError):
        ko.check_vt_from_qkv(drops_last_column, 2, S, 4, 2, 128, CPU, pgen)


# ---------------- wrong operators ----------------
def _rejected(check, *args):
    with pytest.raises(AssertionError) as e:
        check(*args)
    assert not str(e.value).startswith("generator"), e.value   # not a premise


def test_exact_variant_passes_every_check(pgen):
    """The operator the wrong ones are cut from passes, so each rejection
    below is due to the one switched property."""
    for fn in (attn_variant(), attn_variant(tiled="ok")):
        for B, H, Hk in HEAD_CONFIGS:
            for tmap in ko.POINTER_MAPS:
                ko.check_pointer(fn, B, H, Hk, 128, tmap, CPU, pgen)
        ko.check_future_decoy(fn, 2, 4, 2, 128, CPU, pgen)
        for mode in ko.PREFILL_MODES:
            ko.check_prefill_random(fn, mode, 1, 4, 2, 384, CPU, pgen)


@pytest.mark.parametrize("S", [64, 128, 384])
def test_mask_ge_rejected_by_pointer_diag(pgen, S):
    _rejected(ko.check_pointer, attn_variant(mask="ge"), 1, 1, 1, S, "diag", CPU, pgen)


@pytest.mark.parametrize("S", [64, 128, 384])
def test_mask_plus1_rejected_by_future_decoy(pgen, S):
    bad = attn_variant(mask="plus1")
    _rejected(ko.check_future_decoy, bad, 2, 4, 2, S, CPU, pgen)
    # no pointer map can see it: the extra key is 60 nats down
    for tmap in ko.POINTER_MAPS:
        ko.check_pointer(bad, 1, 1, 1, S, tmap, CPU, pgen)


@pytest.mark.parametrize("S", [64, 128, 384])
def test_mask_skipped_on_wave_first_row_rejected_by_future_decoy(pgen, S):
    _rejected(ko.check_future_decoy, attn_variant(mask="skip32"), 2, 4, 2, S, CPU, pgen)


@pytest.mark.parametrize("B,H,Hk", [(2, 4, 2), (1, 6, 2)])
def test_kv_head_mod_rejected_by_pointer(pgen, B, H, Hk):
    bad = attn_variant(kv_map="mod")
    for tmap in ko.POINTER_MAPS:
        _rejected(ko.check_pointer, bad, B, H, Hk, 128, tmap, CPU, pgen)
    ko.check_pointer(bad, 1, 1, 1, 128, "diag", CPU, pgen)   # one head: same map


def test_batch0_rejected_by_pointer(pgen):
    bad = attn_variant(batch0=True)
    for tmap in ko.POINTER_MAPS:
        _rejected(ko.check_pointer, bad, 2, 4, 2, 128, tmap, CPU, pgen)


def test_untransposed_output_rejected(pgen):
    bad = attn_variant(transposed=False)
    _rejected(ko.check_pointer, bad, 1, 1, 1, 128, "diag", CPU, pgen)     # on value
    _rejected(ko.check_pointer, bad, 1, 1, 1, 64, "diag", CPU, pgen)      # on shape
    _rejected(ko.check_prefill_random, bad, "diffuse", 1, 4, 2, 384, CPU, pgen)
    _rejected(ko.check_future_decoy, bad, 2, 4, 2, 128, CPU, pgen)


def test_p_rounded_to_bf16_stays_within_the_bound(pgen):
    """P in bf16 with l summed from the ROUNDED weights is a legitimate
    design (its error is of the size the bound grants): it must pass."""
    ok = attn_variant(p_bf16=True)
    for S in (192, 384):
        for mode in ko.PREFILL_MODES:
            ko.check_prefill_random(ok, mode, 1, 4, 2, S, CPU, pgen)
    ko.check_future_decoy(ok, 2, 4, 2, 128, CPU, pgen)
    for tmap in ko.POINTER_MAPS:
        ko.check_pointer(ok, 2, 4, 2, 128, tmap, CPU, pgen)


@pytest.mark.parametrize("mode", ["stair+3", "stair+7"])
@pytest.mark.parametrize("S", [192, 384, 640])
def test_uncompensated_defer_rejected_by_staircase(pgen, S, mode):
    """Deferred tiles weighted exp(s - m - 8) in O but exp(s - m) in l.  The
    rising staircases put the row's heaviest keys into deferred tiles.  (On
    'stair-7' the deferred tiles hold e^-7 of the weight, so the same slip
    moves the output by 1e-3 max|V|: no bf16-level bound can see it there.)"""
    _rejected(ko.check_prefill_random, attn_variant(tiled="bug"), mode, 1, 4, 2, S, CPU, pgen)


# ---------------- 5. quantized GEMM, grouped GEMM, quantizers, MoE combine ----------------
QGEMM_FN = {"fp8": ops.gemm_bt_fp8, "mx": ops.gemm_bt_mxfp8}
QGEMM_SHAPES = [(128, 128, 128), (130, 140, 640), (17, 384, 256)]
GROUPED_SIZES = [[0, 1, 127, 128, 129, 0, 300, 5], [0, 0, 0, 0, 0, 0, 0, 77], [130, 0, 0, 0],
                 [128, 128]]
QUANT_FP8_SHAPES = [(r, K) for r in (1, 3, 64) for K in (8, 64, 2048, 2056, 4096)]
QUANT_MX_SHAPES = [(r, K) for r in (1, 3, 64) for K in (32, 64, 8192, 8224)]
COMBINE_SHAPES = [(k, H) for k in (1, 2, 3) for H in (8, 264, 2048, 2056)]


# ---- premises ----
@pytest.mark.parametrize("K", [128, 256, 384, 640])
def test_qgemm_probe_columns_cover_boundaries(K):
    cols = ko.qgemm_probe_columns(K)
    assert set(ko.probe_columns(K)) <= set(cols) and 0 in cols and K - 1 in cols
    for step in (16, 32, 64, 128):
        for b in range(step, K, step):
            assert b - 1 in cols and b in cols
    assert len(cols) <= 128                      # one 128-row tile probes them all
    assert set(ko.qgemm_onehot_cols(128, K).tolist()) == set(cols)


@pytest.mark.parametrize("kind", ["fp8", "mx"])
@pytest.mark.parametrize("M,N,K", QGEMM_SHAPES)
def test_qgemm_onehot_expectations_are_exact_bf16(gen, kind, M, N, K):
    """C = a b 2^(..) is a finite, non-zero, NORMAL bf16 value everywhere."""
    args, a64, b64 = ko.make_qgemm_case(kind, "onehot", gen, M, N, K)
    assert int((args[0] != 0).sum()) == M and bool(((args[0] != 0).sum(dim=1) == 1).all())
    c = a64 @ b64.t()
    assert torch.equal(c.to(torch.bfloat16).double(), c)
    assert bool(torch.isfinite(c).all())
    assert float(c.abs().min()) >= 2.0 ** -126 and float(c.abs().max()) < 2.0 ** 127
    s = (torch.cat([args[1], args[3]]).double() if kind == "fp8"
         else torch.exp2(torch.cat([args[1], args[3]]).double() - 127))
    assert bool(ko.is_pow2(s).all())


@pytest.mark.parametrize("M,N,nblk", [(128, 128, 4), (1, 384, 20), (2560, 4352, 12)])
def test_mx_probe_scale_patterns_are_distinct(gen, M, N, nblk):
    """Any two blocks of a row carry different exponents; an A row differs
    from every B row in every block (parity); one A row sits near byte
    127 + 40 and one B row near 127 - 40."""
    a_s, b_s = ko.mx_probe_scales(gen, M, N, nblk)
    for s in (a_s, b_s):
        srt = s.long().sort(dim=1).values
        assert bool((srt[:, 1:] != srt[:, :-1]).all())
    assert bool((a_s.long() % 2 == 1).all()) and bool((b_s.long() % 2 == 0).all())
    assert int(a_s[min(1, M - 1)].min()) >= 127 + 40 - 32
    assert int(a_s[min(1, M - 1)].max()) >= 127 + 40
    assert int(b_s[min(2, N - 1)].max()) <= 127 - 40 + 32
    assert int(b_s[min(2, N - 1)].min()) <= 127 - 40


def test_e4m3_rne_bytes_is_round_to_nearest_even(gen):
    v = ko.all_e4m3_magnitudes()
    assert v.numel() == 127 and float(v[0]) == 0 and float(v[-1]) == 448
    assert bool((v[1:] > v[:-1]).all())
    codes = torch.arange(0, 0x7f, dtype=torch.uint8)
    assert torch.equal(ko.e4m3_rne_bytes(v), codes)                       # identity
    assert torch.equal(ko.e4m3_rne_bytes(-v), codes | 0x80)               # sign kept, -0 too
    mids = (v[:-1] + v[1:]) / 2
    even = torch.where(codes[:-1] % 2 == 0, codes[:-1], codes[1:])        # even code = even mantissa
    assert torch.equal(ko.e4m3_rne_bytes(mids), even)
    assert torch.equal(ko.e4m3_rne_bytes(mids * (1 + 2.0 ** -40)), codes[1:])
    assert torch.equal(ko.e4m3_rne_bytes(mids * (1 - 2.0 ** -40)), codes[:-1])
    assert int(ko.e4m3_rne_bytes(torch.tensor([463.9], dtype=torch.float64))) == 0x7e
    # and it agrees with torch's conversion wherever that rounds an f32 once
    x = (torch.randn(20000, generator=gen) * torch.exp2(torch.randint(-12, 8, (20000,), generator=gen)
                                                         .float())).clamp(-448, 448)
    assert torch.equal(ko.e4m3_rne_bytes(x.double()),
                       x.to(torch.float8_e4m3fn).view(torch.uint8))
    lo, hi = ko.e4m3_neighbours(torch.tensor([0.0, 17.0, 448.0, 2.0 ** -10, 15.9],
                                             dtype=torch.float64))
    assert lo.tolist() == [0.0, 16.0, 448.0, 0.0, 15.0]
    assert hi.tolist() == [2.0 ** -9, 18.0, 480.0, 2.0 ** -9, 16.0]


def test_mx_special_blocks_hit_the_edges(gen):
    blocks = dict(ko.mx_special_blocks(gen))
    assert len([n for n in blocks if n.startswith("amax at ")]) == 32

    def byte(name):
        return int(ko.quant_mxfp8_expect(blocks[name].reshape(1, 32))[1])

    for j in (-20, 0, 9, 30):
        assert byte(f"0.875*2^{j}") == j - 9 + 127        # amax 2^-e == 448 exactly
        assert byte(f"0.875*2^{j}+ulp") == j - 8 + 127    # one ulp more: steps
        assert byte(f"0.875*2^{j}-ulp") == j - 9 + 127
        assert byte(f"2^{j}") == j - 8 + 127
        assert byte(f"2^{j}-ulp") == j - 8 + 127          # floor gives j - 9, then the step
        q, _ = ko.quant_mxfp8_expect(blocks[f"0.875*2^{j}"].reshape(1, 32))
        assert int(q[0, 5]) == 0x7e                       # 448
    assert byte("zero block") == 0 and byte("subnormal") == 0 and byte("bf16 max") == 247
    q, _ = ko.quant_mxfp8_expect(blocks["subnormal"].reshape(1, 32))
    assert float(ko.e4m3_to_f64(q)[0, 9]) == 5 * 2.0 ** -6   # clamped scale keeps the payload
    for p in range(32):
        b = blocks[f"amax at {p}"].double().abs()
        assert int(b.argmax()) == p and float(b.sort().values[-2]) < float(b[p])
    q, s = ko.quant_mxfp8_expect(blocks["midpoints*2^0"].reshape(1, 32))
    assert int(s) == 127
    got = ko.e4m3_to_f64(q)[0, 1:5].tolist()
    assert got == [16.0, 20.0, 20.0, 24.0]                # 17 19 21 23: ties to even


@pytest.mark.parametrize("rows,K", QUANT_MX_SHAPES)
def test_mx_quant_inputs_plant_everything(gen, rows, K):
    calls = ko.mx_quant_inputs(gen, rows, K)
    nsp = len(ko.mx_special_blocks(gen))
    free = (rows - (1 if rows >= 3 else 0)) * (K // 32)
    assert len(calls) == -(-nsp // free)
    x = torch.cat([c.reshape(-1, 32) for c in calls]).double()
    amax = x.abs().amax(dim=1)
    assert bool((amax == 0).any()) and float(amax.max()) == float(torch.finfo(torch.bfloat16).max)
    assert bool(((amax > 0) & (amax < 2.0 ** -126)).any())            # subnormal block
    if rows >= 3:
        assert all(bool((c[1] == 0).all()) for c in calls)
    if rows * (K // 32) > 2 * nsp:                                     # per-block range
        nz = amax[amax > 0]
        assert float(nz.max() / nz.min()) > 2.0 ** 60


@pytest.mark.parametrize("rows,K", QUANT_FP8_SHAPES)
def test_fp8_quant_tie_cap_holds_for_the_reference(gen, rows, K):
    """At most 0.1% of a call's elements (exact rows aside) lie within
    4 * 2^-24 of an e4m3 midpoint, so the reference needs no more excuses
    than that; every planted position and each exact row is there."""
    calls = ko.fp8_quant_inputs(gen, rows, K)
    seen = set()
    for x, exact in calls:
        s_ref = ko.quant_fp8_scale_ref(x)
        near = ko.fp8_near_midpoint(x, s_ref)
        assert int(near[~exact].sum()) <= int(ko.FP8_TIE_CAP * x.numel())
        seen.update(x.double().abs().argmax(dim=1)[x.double().abs().amax(dim=1) > 0].tolist())
        for r in exact.nonzero().flatten().tolist():
            assert bool(ko.is_pow2(s_ref[r])), "exact row: scale is a power of two"
            t = x[r].double() / s_ref[r].double()
            lo, hi = ko.e4m3_neighbours(t.abs())
            assert bool(((t.abs() == lo) | (t.abs() == (lo + hi) / 2)).all())
            assert bool((t.abs() == (lo + hi) / 2).any()) or K < 64
    assert set(ko.fp8_amax_positions(K)) <= seen
    assert sum(int(e.sum()) for _, e in calls) == 3
    assert any(bool((x.double().abs().amax(dim=1) == 0).any()) for x, _ in calls)
    if K == 2056:
        assert {2048, 2055, 0, 511, 512, 1023, 1024, 1535, 1536, 2047} <= set(
            ko.fp8_amax_positions(K))


def test_grouped_and_combine_generators(gen):
    a, w, starts, ref64, absdot = ko.make_grouped_case(gen, [0, 3, 130], 128, 64, "random")
    assert starts == [0, 0, 3, 133] and a.shape == (133, 64) and w.shape == (3, 128, 64)
    down, pos, wt, ref64, absum = ko.make_combine_case(gen, 7, 3, 264, "random")
    P = 7 * 3 + 5
    assert pos.unique().numel() == 21 and int(pos.max()) < P       # an injection
    pads = sorted(set(range(P)) - set(pos.flatten().tolist()))
    assert len(pads) == 5 and bool((wt[pads] == 0).all()) and bool((wt[pos.long()] > 0).all())
    assert bool((down[pads] == 64).all())
    assert not torch.equal(pos.flatten().long(), torch.arange(21))  # permuted


# ---- the CPU fallbacks pass every new check ----
@pytest.mark.parametrize("kind", ["fp8", "mx"])
@pytest.mark.parametrize("M,N,K", QGEMM_SHAPES)
def test_qgemm_cpu_fallback_passes(gen, kind, M, N, K):
    ko.check_qgemm_onehot(QGEMM_FN[kind], kind, M, N, K, CPU, gen)
    ko.check_qgemm_int(QGEMM_FN[kind], kind, M, N, K, CPU, gen)
    # true fp32 sums need no kfactor (the GPU's is measured, QGEMM_KFACTOR)
    assert ko.check_qgemm_random(QGEMM_FN[kind], kind, M, N, K, CPU, gen, kfactor=1) <= 1.0


@pytest.mark.parametrize("sizes", GROUPED_SIZES)
def test_grouped_gemm_cpu_fallback_passes(gen, sizes):
    for N, K in ((128, 64), (384, 192)):
        ko.check_grouped_gemm(ops.grouped_gemm_bt, sizes, N, K, CPU, gen)


def test_grouped_gemm_rejects_offsets_past_the_rows(gen):
    a, w = ko.rand_bf16(gen, 10, 64), ko.rand_bf16(gen, 2, 128, 64)
    with pytest.raises(ValueError):
        ops.grouped_gemm_bt(a, w, [0, 4, 11])
    with pytest.raises(ValueError):
        ops.grouped_gemm_bt(a, w, [0, 4])          # E + 1 offsets, no fewer
    with pytest.raises(ValueError):
        ops.grouped_gemm_bt(a, w, [0, 6, 4])
    assert ops.grouped_gemm_bt(a, w, [0, 4, 10]).shape == (10, 128)


@pytest.mark.parametrize("rows,K", QUANT_MX_SHAPES)
def test_quant_mxfp8_cpu_fallback_passes(gen, rows, K):
    ko.check_quant_mxfp8(ops.quant_mxfp8, rows, K, CPU, gen)


@pytest.mark.parametrize("rows,K", QUANT_FP8_SHAPES)
def test_quant_fp8_cpu_fallback_passes(gen, rows, K):
    """quant_fp8_ref divides by the scale where the kernel multiplies by its
    rounded inverse; the neighbour rule admits both."""
    ko.check_quant_fp8(ops.quant_fp8, rows, K, CPU, gen)


@pytest.mark.parametrize("k,H", COMBINE_SHAPES)
def test_moe_combine_reference_passes(gen, k, H):
    ko.check_moe_combine(ref.moe_combine_ref, 7, k, H, CPU, gen)


# ---- mutants: each wrong operator is rejected by a named check ----
def qgemm_mutant(kind, name):
    """The CPU fallback with one property of the tiled kernels switched."""
    def fn(a_q, a_s, b_q, b_s):
        M, K = a_q.shape
        N = b_q.shape[0]
        if name == "drop_last_tile":              # the K loop ends one tile early
            a_q = a_q.clone()
            a_q[:, K - 128:] = 0
        elif name == "stale_last_scales":         # na / nb never copied for the last tile
            a_s, b_s = a_s.clone(), b_s.clone()
            a_s[:, -4:], b_s[:, -4:] = a_s[:, -8:-4].clone(), b_s[:, -8:-4].clone()
        elif name == "swap_lhi":                  # the lane halves' blocks exchanged
            a_s = a_s.view(M, -1, 2).flip(-1).reshape(M, -1)
            b_s = b_s.view(N, -1, 2).flip(-1).reshape(N, -1)
        elif name == "swap_halves":               # kk = 0 / 1 scale pairs exchanged
            a_s = a_s.view(M, -1, 2, 2).flip(-2).reshape(M, -1)
            b_s = b_s.view(N, -1, 2, 2).flip(-2).reshape(N, -1)
        elif name == "a_s_by_column":             # epilogue reads a_s[col]
            af = a_q.view(torch.float8_e4m3fn).float()
            bf = b_q.view(torch.float8_e4m3fn).float()
            return ((af @ bf.t()) * a_s[torch.arange(N) % M].unsqueeze(0)
                    * b_s.unsqueeze(0)).to(torch.bfloat16)
        elif name == "swizzle_row_plus1":         # A's LDS chunk XOR taken from row + 1
            r = torch.arange(M)
            x = (r & 7) ^ ((r + 1) & 7)
            c = torch.arange(8).unsqueeze(0) ^ x.unsqueeze(1)           # [M, 8]
            idx = c.view(M, 1, 8, 1).expand(M, K // 128, 8, 16)
            a_q = a_q.view(M, K // 128, 8, 16).gather(2, idx).reshape(M, K)
        else:
            raise ValueError(name)
        return QGEMM_FN[kind](a_q, a_s, b_q, b_s)
    return fn


QG = (130, 140, 384)


@pytest.mark.parametrize("kind", ["fp8", "mx"])
def test_dropped_last_k_tile_rejected(gen, kind):
    bad = qgemm_mutant(kind, "drop_last_tile")
    _rejected(ko.check_qgemm_onehot, bad, kind, *QG, CPU, gen)
    _rejected(ko.check_qgemm_int, bad, kind, *QG, CPU, gen)
    _rejected(ko.check_qgemm_random, bad, kind, *QG, CPU, gen)


def test_stale_last_tile_scales_rejected(gen):
    bad = qgemm_mutant("mx", "stale_last_scales")
    _rejected(ko.check_qgemm_onehot, bad, "mx", *QG, CPU, gen)
    _rejected(ko.check_qgemm_random, bad, "mx", *QG, CPU, gen)
    _rejected(ko.check_qgemm_onehot, bad, "mx", 128, 128, 256, CPU, gen)


@pytest.mark.parametrize("name", ["swap_lhi", "swap_halves"])
@pytest.mark.parametrize("K", [128, 384])
def test_swapped_mx_scale_blocks_rejected(gen, name, K):
    _rejected(ko.check_qgemm_onehot, qgemm_mutant("mx", name), "mx", 128, 128, K, CPU, gen)


def test_a_scale_indexed_by_column_rejected(gen):
    bad = qgemm_mutant("fp8", "a_s_by_column")
    _rejected(ko.check_qgemm_onehot, bad, "fp8", *QG, CPU, gen)
    _rejected(ko.check_qgemm_int, bad, "fp8", *QG, CPU, gen)
    _rejected(ko.check_qgemm_random, bad, "fp8", *QG, CPU, gen)


@pytest.mark.parametrize("kind", ["fp8", "mx"])
def test_chunk_swizzle_off_by_one_row_rejected(gen, kind):
    bad = qgemm_mutant(kind, "swizzle_row_plus1")
    _rejected(ko.check_qgemm_onehot, bad, kind, *QG, CPU, gen)
    _rejected(ko.check_qgemm_int, bad, kind, *QG, CPU, gen)


def grouped_mutant(name):
    def fn(a, w, seg):
        starts, E = list(seg), w.shape[0]
        if name == "expert_plus1":                # a tile takes its neighbour's weights
            return ops.grouped_gemm_bt(a, torch.roll(w, -1, 0), seg)
        out = ops.grouped_gemm_bt(a, w, seg)
        if name == "mask_gt":                     # row == seg_end stored by the tile before it
            for e in range(E):
                s, t = starts[e], starts[e + 1]
                if t > s and (t - s) % 128 and t < a.shape[0]:
                    out[t] = ref.gemm_bt_ref(a[t:t + 1], w[e])
        return out
    return fn


@pytest.mark.parametrize("name", ["mask_gt", "expert_plus1"])
@pytest.mark.parametrize("sizes", [GROUPED_SIZES[0], [130, 0, 0, 5]])
def test_grouped_gemm_mutants_rejected(gen, name, sizes):
    _rejected(ko.check_grouped_gemm, grouped_mutant(name), sizes, 128, 64, CPU, gen)


def test_mx_scale_without_the_step_rejected(gen):
    def floor_only(x):                            # OCP floor - 8, saturating
        blk = x.float().view(x.shape[0], -1, 32)
        amax = blk.abs().amax(dim=-1)
        e = torch.where(amax > 0, torch.frexp(amax)[1].float() - 9,
                        torch.full_like(amax, -127.0)).clamp(-127, 127)
        q = (blk * torch.exp2(-e).unsqueeze(-1)).clamp(-448, 448)
        return (q.to(torch.float8_e4m3fn).view(torch.uint8).reshape(x.shape),
                (e + 127).to(torch.uint8))

    for rows, K in ((1, 32), (3, 64), (64, 8224)):
        _rejected(ko.check_quant_mxfp8, floor_only, rows, K, CPU, gen)


def test_fp8_quant_mutants_rejected(gen):
    def truncating(x):                            # round toward zero
        q, s = ref.quant_fp8_ref(x)
        t = (x.float() / s.unsqueeze(1)).double()
        lo, _ = ko.e4m3_neighbours(t.abs().clamp(max=448))
        return ko._e4m3_encode(lo, torch.signbit(t)), s

    def scale_by_reciprocal(x):                   # amax * (1 / 448): not amax / 448
        q, s = ref.quant_fp8_ref(x)
        amax = x.float().abs().amax(dim=-1)
        return q, torch.where(amax > 0, amax * (torch.tensor(1.0) / 448.0), s)

    def off_by_one_code(x):                       # the farther neighbour, one element
        q, s = ref.quant_fp8_ref(x)
        q = q.clone()
        big = x.double().abs().argmax(dim=1)      # the row maximum: code 0x7e
        q[0, big[0]] -= 1
        return q, s

    for rows, K in ((1, 64), (3, 2056), (64, 4096)):
        _rejected(ko.check_quant_fp8, truncating, rows, K, CPU, gen)
        _rejected(ko.check_quant_fp8, off_by_one_code, rows, K, CPU, gen)
    _rejected(ko.check_quant_fp8, scale_by_reciprocal, 64, 64, CPU, gen)


@pytest.mark.parametrize("k,H", COMBINE_SHAPES)
def test_combine_ignoring_last_term_rejected(gen, k, H):
    def bad(down, pos, weight):
        if k == 1:
            return torch.zeros(pos.shape[0], H, dtype=torch.bfloat16)
        return ref.moe_combine_ref(down, pos[:, :k - 1], weight)

    _rejected(ko.check_moe_combine, bad, 7, k, H, CPU, gen)


def test_combine_using_a_pad_row_rejected(gen):
    def bad(down, pos, weight):                   # weight taken by position, not by slot
        w = torch.ones_like(weight)
        return ref.moe_combine_ref(down, pos, w)

    _rejected(ko.check_moe_combine, bad, 7, 2, 264, CPU, gen)


# ---------------- dense bf16 GEMM ----------------
GEMM_CPU_SHAPES = [(128, 128, 64), (256, 256, 256), (384, 640, 320), (17, 256, 128)]
GM = (256, 256, 256)      # mutants: square, 2 x 2 output tiles of 128, 4 K-tiles of 64
GEMM_CHECKS = {"onehot_a": lambda fn, *a: ko.check_gemm_onehot(fn, *a, sides=("a",)),
               "onehot_b": lambda fn, *a: ko.check_gemm_onehot(fn, *a, sides=("b",)),
               "int": ko.check_gemm_int,
               "random": ko.check_gemm_random}


@pytest.mark.parametrize("K", [64, 128, 192, 256, 320, 384, 512, 640])
def test_gemm_probe_columns_cover_boundaries(K):
    cols = ko.gemm_probe_columns(K)
    assert cols[0] == 0 and cols[-1] == K - 1 and cols == sorted(set(cols))
    for step in (8, 16, 32, 64, 128):
        for b in range(step, K, step):
            assert b - 1 in cols and b in cols
    # every 8-element chunk of every K-tile holds a probe
    assert {c // 8 for c in cols} == set(range(K // 8))
    # the rows of the smallest tile visit all of them in the calls made
    for rows in (17, 128, 256):
        seen = set()
        for call in range(ko.gemm_onehot_ncalls(rows, K)):
            seen |= set(ko.gemm_onehot_operand(torch.Generator().manual_seed(1), rows, K,
                                               call)[1].tolist())
        assert seen == set(cols)


def test_gemm_onehot_operand_is_onehot_pow2(gen):
    x, col, val = ko.gemm_onehot_operand(gen, 300, 640)
    assert bool(((x != 0).sum(dim=1) == 1).all())
    assert torch.equal(x[torch.arange(300), col].double(), val)
    assert bool(ko.is_pow2(val.abs()).all()) and bool((val < 0).any()) and bool((val > 0).any())
    assert float(val.abs().min()) >= 2.0 ** -3 and float(val.abs().max()) <= 2.0 ** 3


def test_gemm_int_sums_stay_exact_in_fp32(gen):
    """At the largest K and the largest shape of the GPU file: the fp32 CPU
    matmul that serves as the expectation equals the fp64 one."""
    a, b = ko.gemm_int_operands(gen, 256, 384, 640)
    assert float(ko.gemv_abs_dot(a, b.double()).max()) < 2 ** 24
    assert torch.equal((a.float() @ b.float().t()).double(), a.double() @ b.double().t())
    for t in (a, b):      # every row differs from every other: tiles are distinguishable
        assert torch.unique(t, dim=0).shape[0] == t.shape[0]


@pytest.mark.parametrize("M,N,K", GEMM_CPU_SHAPES)
def test_gemm_fp32_reference_passes_every_check(gen, M, N, K):
    """The correct fp32-accumulating operator (and ops.gemm_bt's CPU route,
    which is the same thing) passes all three checks at kfactor 1."""
    for fn in (ref.gemm_bt_ref, ops.gemm_bt, ops.gemm_bt_tiled):
        assert ko.check_gemm_all(fn, M, N, K, CPU, gen) <= 1.0


def gemm_mutant(name, operand="a"):
    """ref.gemm_bt_ref with one property of a tiled kernel switched.  The K
    mutants act on tile 1 (of 64) of one operand, as a fault in that
    operand's LDS buffer would; the output mutants on 128 x 128 tiles."""
    def permute_k(x, idx):
        return x[:, idx]

    def fn(a, b):
        K = a.shape[1]
        k = torch.arange(K)
        if name in ("drop_k_tile", "swap_chunks", "swap_khalves"):
            if name == "drop_k_tile":               # the K loop skips a tile
                keep = ((k < 64) | (k >= 128)).to(a.dtype)
                mut = lambda x: x * keep
            elif name == "swap_chunks":             # chunks 2 and 5 of tile 1 exchanged
                idx = k.clone()
                idx[80:88], idx[104:112] = k[104:112], k[80:88]
                mut = lambda x: permute_k(x, idx)
            else:                                   # the ^64-byte k-half offset inverted
                idx = k.clone()
                idx[64:96], idx[96:128] = k[96:128], k[64:96]
                mut = lambda x: permute_k(x, idx)
            a, b = (mut(a), b) if operand == "a" else (a, mut(b))
            return ref.gemm_bt_ref(a, b)
        if name == "double_k_tile":                 # a buffer-parity slip: tile 1 read twice
            c = a.float() @ b.float().t() + a[:, 64:128].float() @ b[:, 64:128].float().t()
            return c.to(a.dtype)
        c = ref.gemm_bt_ref(a, b)
        if name == "swap_out_tiles":                # a hole in the workgroup remap
            c = c.clone()
            t = c[:128, :128].clone()
            c[:128, :128] = c[128:256, 128:256]
            c[128:256, 128:256] = t
        elif name == "dup_out_tile":                # two workgroups on one tile
            c = c.clone()
            c[128:256, :128] = c[:128, :128]
        elif name == "transposed":
            c = c.t().contiguous()
        elif name == "one_ulp":
            c = c.clone()
            c[200, 77] = _next_bf16(c[200, 77])
        else:
            raise ValueError(name)
        return c
    return fn


def test_gemm_mutants_are_cut_from_a_passing_operator(gen):
    for check in GEMM_CHECKS.values():
        check(ref.gemm_bt_ref, *GM, CPU, gen)


@pytest.mark.parametrize("check", ["onehot_a", "onehot_b", "int", "random"])
@pytest.mark.parametrize("operand", ["a", "b"])
@pytest.mark.parametrize("name", ["drop_k_tile", "swap_chunks", "swap_khalves"])
def test_gemm_k_tile_mutants_rejected_by_onehot_int_and_random(gen, name, operand, check):
    _rejected(GEMM_CHECKS[check], gemm_mutant(name, operand), *GM, CPU, gen)


@pytest.mark.parametrize("check", ["onehot_a", "onehot_b", "int", "random"])
@pytest.mark.parametrize("name", ["double_k_tile", "swap_out_tiles", "dup_out_tile",
                                  "transposed"])
def test_gemm_tile_mutants_rejected_by_onehot_int_and_random(gen, name, check):
    _rejected(GEMM_CHECKS[check], gemm_mutant(name), *GM, CPU, gen)


@pytest.mark.parametrize("check", ["onehot_a", "onehot_b", "int"])
def test_gemm_one_ulp_rejected_by_onehot_and_int(gen, check):
    """One element off by one bf16 ulp fails both bit-exact checks (the
    random check allows half an ulp of rounding and cannot see it)."""
    _rejected(GEMM_CHECKS[check], gemm_mutant("one_ulp"), *GM, CPU, gen)


# ---------------- elementwise ops ----------------
ELEM_HIDDEN = [8, 2040, 2048, 2056]


def _cpu_add(a, b):
    return (a.float() + b.float()).to(torch.bfloat16)


def _cpu_fused(x, res, w, eps):
    y = ops.fused_add_rmsnorm(x, res, w, eps)
    return y, res


def _cpu_swiglu_padded(gu, out_rows):
    return ops.swiglu(gu, out_rows=out_rows)


def test_bf16_rne64_rounds_once_to_nearest_even(gen):
    v = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 3 * 2.0 ** -8,
                      -(1.0 + 2.0 ** -8), 255.5, 0.0, 2.0 ** -100 * (1 + 2.0 ** -8)],
                     dtype=torch.float64)
    exp = [1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, -1.0, 256.0, 0.0, 2.0 ** -100]
    assert ko.bf16_rne64(v).double().tolist() == exp
    # 1 + 2^-8 + 2^-40 through fp32 first would lose the 2^-40 and tie down to 1
    assert float(v[1].float().to(torch.bfloat16)) == 1.0
    x = torch.randn(4096, generator=gen, dtype=torch.float64).float().double()
    assert torch.equal(ko.bf16_rne64(x), x.float().to(torch.bfloat16))


@pytest.mark.parametrize("n", [8, 2048, 8 * 256 * 3 + 8])
def test_cpu_add_passes(gen, n):
    ko.check_add_bf16(_cpu_add, n, CPU, gen)


@pytest.mark.parametrize("hidden", ELEM_HIDDEN)
@pytest.mark.parametrize("rows", [1, 3])
def test_cpu_rmsnorm_fallbacks_pass(gen, rows, hidden):
    ko.check_rmsnorm(ops.rmsnorm, rows, hidden, CPU, gen)
    ko.check_fused_add_rmsnorm(_cpu_fused, rows, hidden, CPU, gen)


@pytest.mark.parametrize("inter", [8, 2040, 2056])
@pytest.mark.parametrize("rows", [0, 1, 3])
def test_cpu_swiglu_fallback_passes(gen, rows, inter):
    ko.check_swiglu(ops.swiglu, _cpu_swiglu_padded, rows, inter, CPU, gen)


@pytest.mark.parametrize("Hq,Hk", [(1, 1), (6, 2)])
@pytest.mark.parametrize("D", [32, 128, 256])
def test_cpu_rope_inplace_fallback_passes(gen, D, Hq, Hk):
    ko.check_rope_inplace(ops.rope_inplace, Hq, Hk, D, CPU, gen, ref.rope_tables)


def test_elementwise_checks_catch_wrong_kernels(gen):
    def add_truncating(a, b):                       # rounds toward zero
        s = (a.float() + b.float()).view(torch.int32) & ~0xFFFF
        return s.view(torch.float32).to(torch.bfloat16)

    def add_drops_last_vector(a, b):                # n8 rounded down to the block
        c = _cpu_add(a, b)
        c[-8:] = 0
        return c

    _rejected(ko.check_add_bf16, add_truncating, 8, CPU, gen)
    _rejected(ko.check_add_bf16, add_drops_last_vector, 2056, CPU, gen)

    def norm_unrounded_residual(x, res, w, eps):    # y from the fp32 sum, res_out one ulp off
        y, r = _cpu_fused(x, res.clone(), w, eps)
        r[0, 0] = _next_bf16(r[0, 0])
        return y, r

    def norm_mean_over_2048(x, w, eps):             # hidden rounded down to 256 threads x 8
        h = max(8, x.shape[-1] // 2048 * 2048)
        xf = x.float()
        ms = xf[:, :h].pow(2).sum(-1, keepdim=True) / x.shape[-1]
        return (xf * torch.rsqrt(ms + eps) * w.float()).to(x.dtype)

    def norm_w_shifted(x, w, eps):                  # second pass reads w one vector late
        return ops.rmsnorm(x, torch.roll(w, 8), eps)

    _rejected(ko.check_fused_add_rmsnorm, norm_unrounded_residual, 3, 2056, CPU, gen)
    _rejected(ko.check_rmsnorm, norm_mean_over_2048, 3, 2056, CPU, gen)
    _rejected(ko.check_rmsnorm, norm_w_shifted, 1, 2056, CPU, gen)

    def swiglu_bf16_silu(gu):                       # silu rounded to bf16 before * up
        i = gu.shape[-1] // 2
        s = torch.nn.functional.silu(gu[..., :i].float()).to(torch.bfloat16)
        return (s.float() * gu[..., i:].float()).to(torch.bfloat16)

    def pad_not_zeroed(gu, out_rows):
        y = _cpu_swiglu_padded(gu, out_rows)
        if out_rows > gu.shape[0]:
            y[-1, -1] = -0.0
        return y

    _rejected(ko.check_swiglu, swiglu_bf16_silu, _cpu_swiglu_padded, 3, 2056, CPU, gen)
    _rejected(ko.check_swiglu, ops.swiglu, pad_not_zeroed, 3, 2056, CPU, gen)

    def rope_wrong_sign(q, k, cs, pos):             # rotates the other way
        cs = cs.clone()
        cs[:, cs.shape[1] // 2:] *= -1
        ops.rope_inplace(q, k, cs, pos)

    def rope_skips_k(q, k, cs, pos):
        ops.rope_inplace(q, k.clone(), cs, pos)

    _rejected(ko.check_rope_inplace, rope_wrong_sign, 6, 2, 128, CPU, gen, ref.rope_tables)
    _rejected(ko.check_rope_inplace, rope_skips_k, 6, 2, 128, CPU, gen, ref.rope_tables)


def test_gemm_dropped_row_of_padding_rejected(gen):
    """An operator that returns the padded row count fails on the shape."""
    def bad(a, b):
        c = ref.gemm_bt_ref(a, b)
        return torch.nn.functional.pad(c, (0, 0, 0, (-c.shape[0]) % 128))

    for check in GEMM_CHECKS.values():
        _rejected(check, bad, 17, 256, 128, CPU, gen)
