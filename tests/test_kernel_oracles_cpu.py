"""CPU checks of the decode-kernel oracles (tests/kernel_oracles.py).

Three things are established without a GPU:
1. each fp64 oracle agrees with the existing fp32 reference in
   senweaver_amd.ops.reference on random data;
2. every input generator satisfies the condition its GPU test relies on
   (score gap, integer-sum magnitude, power-of-two scales, exact
   representability of the bit-exact expectations);
3. the ops.* CPU fallbacks pass the same edge cases the GPU kernels get.
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


@pytest.mark.parametrize("kind,K", [("bf16", 14336), ("bf16", 15360), ("fp8", 4096), ("mx", 4096)])
def test_integer_sums_stay_exact_in_fp32(gen, kind, K):
    """sum |x||w| (an upper bound on every partial sum in any order), in
    units of the smallest scale 2^-3, stays below 2^24."""
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
