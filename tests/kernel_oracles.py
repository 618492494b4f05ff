"""fp64 oracles, input generators and error bounds for the decode kernels,
the prefill attention kernels, the tiled quantized GEMMs (fp8 / mxfp8), the
grouped GEMM, the quantizers and moe_combine, the dense bf16 GEMM kernels
and the elementwise kernels.

Helper module for test_kernel_oracles_cpu.py, test_decode_edges_gpu.py,
test_prefill_edges_gpu.py, test_quant_gemm_edges_gpu.py,
test_gemm_edges_gpu.py and test_elemwise_edges_gpu.py (no tests live
here).  Every oracle takes the
SAME bf16 / uint8 tensors the kernel gets, upcasts with ``.double()`` and computes in plain torch on the
CPU, so the only error in an oracle is fp64 rounding (~1e-16 relative).

Bounds are derived from the number formats, never from kernel output:

* bf16 has 8 significand bits, so rounding a result r to bf16 (RNE) moves
  it by at most half an ulp, which lies between 2^-9 |r| (r just below a
  power of two) and 2^-8 |r| (just above); the bounds allow 2^-8 |r|.
* fp32 accumulation of K exact products in ANY order is off by at most
  (K-1) 2^-24 sum|x_k w_k| to first order (bf16 x bf16 and e4m3 x bf16
  products are exact in fp32: 8+8 and 4+8 significand bits).
"""

from __future__ import annotations

import math

import torch

BF16 = torch.bfloat16
U_BF16_OUT = 2.0 ** -8   # bf16 unit roundoff: half an ulp <= 2^-8 |r|
U_FP32 = 2.0 ** -24      # fp32 unit roundoff


# --------------------------------------------------------------------------
# bit-level comparison
# --------------------------------------------------------------------------
def bits(t: torch.Tensor) -> torch.Tensor:
    """bf16 tensor -> its int16 bit pattern on the CPU (NaN / -0 aware)."""
    assert t.dtype == BF16
    return t.detach().cpu().contiguous().view(torch.int16)


def assert_bits_equal(got: torch.Tensor, exp: torch.Tensor, what: str = ""):
    assert got.shape == exp.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(exp.shape)}"
    g, e = bits(got), bits(exp)
    if torch.equal(g, e):
        return
    bad = (g != e).nonzero()
    i = tuple(int(v) for v in bad[0])
    raise AssertionError(
        f"{what}: {bad.shape[0]} of {g.numel()} elements differ bitwise; first at "
        f"{i}: got {float(got.detach().cpu()[i])!r} expected {float(exp.detach().cpu()[i])!r}")


def assert_within(got: torch.Tensor, ref64: torch.Tensor, bound: torch.Tensor, what: str = ""):
    """|got - ref64| <= bound elementwise (bound broadcastable); NaN fails."""
    err = (got.detach().cpu().double() - ref64).abs()
    ok = err <= bound  # NaN compares False
    if bool(ok.all()):
        return
    bad = (~ok).nonzero()
    i = tuple(int(v) for v in bad[0])
    b = bound.expand_as(err) if isinstance(bound, torch.Tensor) else torch.full_like(err, bound)
    raise AssertionError(
        f"{what}: {bad.shape[0]} of {err.numel()} elements out of bound; first at {i}: "
        f"got {float(got.detach().cpu().double()[i])!r} ref {float(ref64[i])!r} "
        f"err {float(err[i]):.3e} bound {float(b[i]):.3e}")


def rel_fro(got: torch.Tensor, ref64: torch.Tensor) -> float:
    g = got.detach().cpu().double()
    return float((g - ref64).norm() / ref64.norm())


# --------------------------------------------------------------------------
# GEMV family
# --------------------------------------------------------------------------
def probe_columns(K: int) -> list:
    """One-hot probe columns: lane 0 / lane 63 of the first iteration, both
    8-wide halves of the fp8 16-byte step, loop-iteration (512) and step
    (1024) boundaries, LDS ring wrap (slot 6 = column 3072) and the tail."""
    cand = [0, 7, 8, 15, 16, 511, 512, 1023, 1024, 3071, 3072,
            K - 1024, K - 513, K - 512, K - 1]
    return sorted({c for c in cand if 0 <= c < K})


def onehot_calls(M: int, K: int) -> list:
    """Probe columns spread over the rows of ceil(P/M) calls: call c, row m
    probes P[(c*M + m) % P], so every probe is seen at this M."""
    P = probe_columns(K)
    ncalls = -(-len(P) // M)
    return [[P[(c * M + m) % len(P)] for m in range(M)] for c in range(ncalls)]


def onehot_x(cols: list, K: int) -> torch.Tensor:
    x = torch.zeros(len(cols), K, dtype=BF16)
    for m, k in enumerate(cols):
        x[m, k] = 1.0
    return x


def rand_bf16(gen: torch.Generator, *shape) -> torch.Tensor:
    return torch.randn(*shape, generator=gen).to(BF16)


def int_x(gen: torch.Generator, M: int, K: int) -> torch.Tensor:
    """Integers in [-2, 2] as bf16 (exact)."""
    return torch.randint(-2, 3, (M, K), generator=gen).to(BF16)


def _rand_e4m3_bytes(gen, N, K) -> torch.Tensor:
    """Random finite NON-ZERO e4m3fn bytes: magnitude code in [1, 0x7e]
    (0x7f is NaN; +-0 is left out because a one-hot product with -0 would
    be expected as -0 while an fp32 accumulator started at +0 gives +0)."""
    mag = torch.randint(1, 0x7f, (N, K), generator=gen)
    sign = torch.randint(0, 2, (N, K), generator=gen)
    return (mag | (sign << 7)).to(torch.uint8)


def _int_e4m3_bytes(gen, N, K) -> torch.Tensor:
    """Integers in [-4, 4] as e4m3 bytes (integers <= 16 are exact)."""
    w = torch.randint(-4, 5, (N, K), generator=gen).float()
    return w.to(torch.float8_e4m3fn).view(torch.uint8)


def e4m3_to_f64(q: torch.Tensor) -> torch.Tensor:
    return q.cpu().view(torch.float8_e4m3fn).float().double()


def dequant_fp8_ref64(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """Row-scaled e4m3 weights -> fp64 [N, K]."""
    return e4m3_to_f64(q) * s.cpu().double().unsqueeze(1)


def dequant_mx_ref64(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """MX weights (e4m3 bytes + e8m0 byte per 32-block) -> fp64 [N, K]."""
    N, K = q.shape
    f = e4m3_to_f64(q).view(N, K // 32, 32)
    sc = torch.exp2(s.cpu().double() - 127.0).unsqueeze(-1)
    return (f * sc).reshape(N, K)


def make_weights(kind: str, gen: torch.Generator, N: int, K: int, mode: str):
    """Weights for one GEMV kernel family.

    kind: 'bf16' | 'fp8' | 'mx'.  mode: 'random' (unsymmetric random data;
    fp8 row scales are powers of two), 'random_scale' (fp8 only: arbitrary
    positive row scales), 'int' (integers in [-4, 4], power-of-two scales).
    Returns (wargs, w64): the tensors the kernel takes after x, and the
    dequantized fp64 weight matrix [N, K].  Quantized forms are built
    directly from bytes — the quantizer kernels are not involved.
    """
    if kind == "bf16":
        w = (torch.randint(-4, 5, (N, K), generator=gen).to(BF16) if mode == "int"
             else rand_bf16(gen, N, K))
        return (w,), w.double()
    q = _int_e4m3_bytes(gen, N, K) if mode == "int" else _rand_e4m3_bytes(gen, N, K)
    if kind == "fp8":
        if mode == "random_scale":
            s = (2.0 ** -4) * (1.0 + torch.rand(N, generator=gen))
        else:
            s = torch.exp2(torch.randint(-3, 4, (N,), generator=gen).float())
        s = s.float()
        return (q, s), dequant_fp8_ref64(q, s)
    if kind == "mx":
        # e8m0 byte = exponent + 127; 2^-2 .. 2^2 keeps integer sums exact
        s = torch.randint(125, 130, (N, K // 32), generator=gen).to(torch.uint8)
        return (q, s), dequant_mx_ref64(q, s)
    raise ValueError(kind)


def is_pow2(t: torch.Tensor) -> torch.Tensor:
    m, _ = torch.frexp(t.double())
    return m == 0.5


def gemv_ref64(x: torch.Tensor, w64: torch.Tensor) -> torch.Tensor:
    """C[M,N] = x @ w^T in fp64; w is a bf16 tensor or an fp64 dequant."""
    return x.cpu().double() @ w64.cpu().double().t()


def gemv_abs_dot(x: torch.Tensor, w64: torch.Tensor) -> torch.Tensor:
    """(|x| . |w|^T): the scale of the fp32 summation error term."""
    return x.cpu().double().abs() @ w64.cpu().double().abs().t()


def gemv_bound(ref64: torch.Tensor, absdot: torch.Tensor, K: int, kfactor: int = 1) -> torch.Tensor:
    """2^-8 |ref| (bf16 output rounding: half an ulp never exceeds it) +
    kfactor*K 2^-24 (|x|.|w|^T) (worst-case fp32 summation error, any order)."""
    return U_BF16_OUT * ref64.abs() + kfactor * K * U_FP32 * absdot


def exact_bf16(ref64: torch.Tensor) -> torch.Tensor:
    """bf16_rne of an fp64 value that is exactly representable in fp32 (so
    the double -> float -> bf16 chain rounds once).  Asserts that premise."""
    f = ref64.float()
    assert torch.equal(f.double(), ref64), "value is not exact in fp32"
    return f.to(BF16)


def gemv_norm_ref64(x, res, normw, b, eps):
    """Fused add + RMSNorm + GEMV as the kernel defines it: t = x + res is
    NOT rounded; C = (sum_k t normw b) * rsqrt(mean(t^2) + eps);
    res_out = bf16(x + res) computed in fp32.  Returns (C64, res_out_bf16,
    absdot64) with absdot = (|t| |normw| . |b|^T) * rsqrt(mean(t^2)+eps)."""
    xd = x.cpu().double()
    t = xd + res.cpu().double() if res is not None else xd
    rs = torch.rsqrt((t * t).mean(dim=1, keepdim=True) + eps)
    tw = t * normw.cpu().double()
    c = (tw @ b.cpu().double().t()) * rs
    absdot = (tw.abs() @ b.cpu().double().abs().t()) * rs
    if res is not None:
        res_out = (x.cpu().float() + res.cpu().float()).to(BF16)
    else:
        res_out = x.cpu().clone()
    return c, res_out, absdot


def swiglu_ref64(gateup: torch.Tensor) -> torch.Tensor:
    """silu(g) * u in fp64, unrounded.  gateup [M, 2K] -> [M, K]."""
    gu = gateup.cpu().double()
    K = gu.shape[-1] // 2
    g, u = gu[..., :K], gu[..., K:]
    return g * torch.sigmoid(g) * u


def swiglu_onehot_gateup(gen, k: int, K: int) -> torch.Tensor:
    """gateup [1, 2K] whose activation is exactly 32 e_k: u = e_k, g random
    with g_k = 32.  In fp32 1 + exp(-32) == 1, so silu(32) == 32 exactly."""
    g = rand_bf16(gen, 1, K)
    g[0, k] = 32.0
    u = torch.zeros(1, K, dtype=BF16)
    u[0, k] = 1.0
    return torch.cat([g, u], dim=1)


# --------------------------------------------------------------------------
# Paged decode attention
# --------------------------------------------------------------------------
PAGE = 16
NSPLIT = 8


def probe_positions(ctx: int) -> list:
    """Spike positions: page / 32-batch boundaries, both sides of the first
    split boundary, a wave's second and third pass, and the last position."""
    chunk = -(-ctx // NSPLIT)
    cand = [0, 15, 16, 31, 32, chunk - 1, chunk, chunk + 127, chunk + 128, ctx - 1]
    return sorted({p for p in cand if 0 <= p < ctx})


def make_paged_case(gen, ctxs, H, Hk, D=128, qscale=1.0, spare_pages=5, spare_cols=3):
    """Random paged-KV decode case.  Block tables are a random permutation
    of the page pool (unused entries -1, max_pages larger than needed).
    Returns dict(q, kcache, vcache, block_table, ctx_lens, scale)."""
    B = len(ctxs)
    need = [-(-c // PAGE) for c in ctxs]
    P = sum(need) + spare_pages
    perm = torch.randperm(P, generator=gen)
    max_pages = max(need) + spare_cols
    bt = torch.full((B, max_pages), -1, dtype=torch.int32)
    o = 0
    for b in range(B):
        bt[b, :need[b]] = perm[o:o + need[b]].to(torch.int32)
        o += need[b]
    q = (torch.randn(B, H, D, generator=gen) * qscale).to(BF16)
    kc = rand_bf16(gen, P, PAGE, Hk, D)
    vc = rand_bf16(gen, P, PAGE, Hk, D)
    return dict(q=q, kcache=kc, vcache=vc, block_table=bt,
                ctx_lens=torch.tensor(ctxs, dtype=torch.int32),
                scale=1.0 / math.sqrt(D))


def slots_of(block_table_row: torch.Tensor, ctx: int) -> torch.Tensor:
    p = torch.arange(ctx)
    return block_table_row.long()[p // PAGE] * PAGE + (p % PAGE)


def paged_decode_attn_ref64(q, kcache, vcache, block_table, ctx_lens, scale):
    """Gathers slots through the block table; softmax in fp64.  -> [B,H,D] f64"""
    q, kcache, vcache = q.cpu(), kcache.cpu(), vcache.cpu()
    B, H, D = q.shape
    P, _, Hk, _ = kcache.shape
    rep = H // Hk
    kf = kcache.double().reshape(P * PAGE, Hk, D)
    vf = vcache.double().reshape(P * PAGE, Hk, D)
    out = torch.empty(B, H, D, dtype=torch.float64)
    for b in range(B):
        sl = slots_of(block_table[b].cpu(), int(ctx_lens[b]))
        kk, vv = kf[sl], vf[sl]
        for h in range(H):
            s = (kk[:, h // rep] @ q[b, h].double()) * scale
            out[b, h] = torch.softmax(s, dim=0) @ vv[:, h // rep]
    return out


def plant_spike(case: dict, b: int, h: int, p_star: int):
    """K[p*] = 16 q[b,h] on head h's kv head (in a CLONE of the K cache).
    Returns (kcache_new, gap, v_row): gap is the fp64 score distance from p*
    to the best other position (inf when ctx == 1); v_row = V[p*] for the
    kv head, which the kernel must return bit for bit when gap is large:
    every other weight is <= exp(-gap), far below half an fp32 ulp."""
    q, kc, vc = case["q"], case["kcache"].clone(), case["vcache"]
    H = q.shape[1]
    P, _, Hk, D = kc.shape
    kvh = h // (H // Hk)
    ctx = int(case["ctx_lens"][b])
    sl = slots_of(case["block_table"][b], ctx)
    kflat = kc.view(P * PAGE, Hk, D)
    kflat[sl[p_star], kvh] = (q[b, h].float() * 16.0).to(BF16)
    s = (kflat[sl, kvh].double() @ q[b, h].double()) * case["scale"]
    others = torch.cat([s[:p_star], s[p_star + 1:]])
    gap = float(s[p_star] - others.max()) if others.numel() else float("inf")
    return kc, gap, vc.view(P * PAGE, Hk, D)[sl[p_star], kvh].clone()


def attn_bound(vcache: torch.Tensor) -> float:
    """2^-8 max|V|.  The output o is a convex combination of V rows, so
    |o| <= max|V| and half a bf16 ulp of o is <= 2^-8 |o|, reaching
    2^-8 max|V| only if |o| == max|V| is a power of two; what is left covers
    the fp32 softmax error (~1e-5 relative at |score| <= 100)."""
    return U_BF16_OUT * float(vcache.double().abs().max())


# --------------------------------------------------------------------------
# RoPE
# --------------------------------------------------------------------------
def rope_ref64(x: torch.Tensor, cos_sin: torch.Tensor, positions: torch.Tensor):
    """Rotate-half RoPE.  x [T,H,D] bf16, cos_sin [max_pos, D] f32 (the table
    the kernel reads).  Returns (out64, bound64) with
    bound = 2^-8 (|a c| + |b s|) per output element."""
    xd = x.cpu().double()
    half = xd.shape[-1] // 2
    cs = cos_sin.cpu().double()[positions.cpu().long()]
    c, s = cs[:, :half].unsqueeze(1), cs[:, half:].unsqueeze(1)
    x1, x2 = xd[..., :half], xd[..., half:]
    out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    bound = U_BF16_OUT * torch.cat([(x1 * c).abs() + (x2 * s).abs(),
                                    (x2 * c).abs() + (x1 * s).abs()], dim=-1)
    return out, bound


SENTINEL = 1.5  # non-zero cache pre-fill: a stray write of anything else shows


# --------------------------------------------------------------------------
# Sampling
# --------------------------------------------------------------------------
def argmax_ref_rows(logits: torch.Tensor) -> torch.Tensor:
    """Lowest index of the maximum over non-NaN entries; 0 if there is none."""
    x = logits.cpu().double()
    x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
    mx = x.max(dim=1, keepdim=True).values
    first = (x == mx).to(torch.int64).argmax(dim=1)  # first True
    return first.to(torch.int32)


def target_logprob_ref64(logits: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    lp = torch.log_softmax(logits.cpu().double(), dim=-1)
    return lp.gather(1, targets.cpu().long().unsqueeze(1)).squeeze(1)


def argmax_edge_rows(gen, vocab: int):
    """Rows of edge cases for argmax_rows at one vocab size.
    Returns (logits [R, vocab] bf16, names)."""
    rows, names = [], []

    def add(name, r):
        rows.append(r)
        names.append(name)

    add("random", rand_bf16(gen, vocab))
    r = rand_bf16(gen, vocab); r[0] = 50.0
    add("max_first", r)
    r = rand_bf16(gen, vocab); r[vocab - 1] = 50.0
    add("max_last", r)
    add("all_equal", torch.full((vocab,), 0.75, dtype=BF16))
    add("all_neg_inf", torch.full((vocab,), float("-inf"), dtype=BF16))
    r = rand_bf16(gen, vocab)
    r[torch.arange(0, vocab, 3)] = float("nan")   # index 0 is NaN
    add("nan_ignored", r)
    r = rand_bf16(gen, vocab); r[vocab - 1] = 50.0; r[0] = float("nan")
    add("nan_first_max_last", r)
    add("all_nan", torch.full((vocab,), float("nan"), dtype=BF16))
    a, b = 8 * 255 + 3, 8 * 256
    if b < vocab:
        # equal maxima in thread 255's first pass and thread 0's second pass
        r = rand_bf16(gen, vocab); r[a] = 50.0; r[b] = 50.0
        add("tie_across_passes", r)
    return torch.stack(rows), names


def target_logprob_edge_rows(gen, vocab: int):
    """Rows of edge cases for target_logprob.  Returns (logits, targets, names);
    every row has a finite target, so every output must be finite."""
    rows, tgts, names = [], [], []

    def add(name, r, t):
        rows.append(r)
        tgts.append(t)
        names.append(name)

    add("random", rand_bf16(gen, vocab), vocab // 2)
    add("x30_tgt_first", (torch.randn(vocab, generator=gen) * 30).to(BF16), 0)
    add("x30_tgt_last", (torch.randn(vocab, generator=gen) * 30).to(BF16), vocab - 1)
    # -inf over the first 16-byte vector (a thread's FIRST element is -inf)
    r = rand_bf16(gen, vocab)
    r[:min(8, vocab - 1)] = float("-inf")
    add("neg_inf_head", r, vocab - 1)
    r = (torch.randn(vocab, generator=gen) * 30).to(BF16)
    mask = torch.rand(vocab, generator=gen) < 0.5
    mask[:min(8, vocab - 1)] = True
    mask[vocab - 1] = False
    r[mask] = float("-inf")
    add("neg_inf_half_x30", r, vocab - 1)
    r = torch.full((vocab,), float("-inf"), dtype=BF16); r[vocab // 2] = 3.0
    add("single_finite", r, vocab // 2)
    r = rand_bf16(gen, vocab); r[0] = float("-inf")
    add("neg_inf_first_tgt_1", r, 1)
    return torch.stack(rows), torch.tensor(tgts, dtype=torch.int32), names


# --------------------------------------------------------------------------
# Check drivers shared by the CPU (ops.* fallbacks) and GPU (HIP kernels)
# test files.  ``fn(x, *wargs) -> [M, N] bf16`` is the op under test.
# --------------------------------------------------------------------------
def _to(dev, ts):
    return tuple(t.to(dev) for t in ts)


def check_gemv_onehot(fn, kind, Ms, Ns, K, dev, gen):
    """Row m of x is one-hot at column k_m: C[m, :] == W[:, k_m] bit for bit
    (0 * w and the sums of zeros are exact; W[:, k] x 1 is a bf16 value)."""
    for N in Ns:
        wargs, w64 = make_weights(kind, gen, N, K, "random")
        wdev = _to(dev, wargs)
        for M in Ms:
            for cols in onehot_calls(M, K):
                got = fn(onehot_x(cols, K).to(dev), *wdev)
                exp = exact_bf16(w64[:, cols].t().contiguous())
                assert_bits_equal(got, exp, f"{kind} one-hot M={M} N={N} K={K} cols={cols}")


def check_gemv_int(fn, kind, Ms, Ns, K, dev, gen):
    """Small-integer data: every fp32 partial sum is an exactly representable
    integer multiple of the smallest scale, whatever the summation order, so
    the output equals bf16_rne(exact sum) bit for bit."""
    for N in Ns:
        wargs, w64 = make_weights(kind, gen, N, K, "int")
        wdev = _to(dev, wargs)
        for M in Ms:
            x = int_x(gen, M, K)
            # premise: |any partial sum| <= sum|x||w| < 2^24 units of 2^-3
            assert float(gemv_abs_dot(x, w64).max()) * 8 < 2 ** 24
            got = fn(x.to(dev), *wdev)
            exp = exact_bf16(gemv_ref64(x, w64))
            assert_bits_equal(got, exp, f"{kind} integer M={M} N={N} K={K}")


def check_gemv_random(fn, kind, Ms, Ns, K, dev, gen, mode="random"):
    for N in Ns:
        wargs, w64 = make_weights(kind, gen, N, K, mode)
        wdev = _to(dev, wargs)
        for M in Ms:
            x = rand_bf16(gen, M, K)
            got = fn(x.to(dev), *wdev)
            ref = gemv_ref64(x, w64)
            assert_within(got, ref, gemv_bound(ref, gemv_abs_dot(x, w64), K),
                          f"{kind} random M={M} N={N} K={K}")


def check_gemv_norm(fn, Ms, Ns, K, dev, gen, with_res, onehot=False, eps=1e-5,
                    fro_tol=None):
    """fn(x, res, normw, b, eps) -> (C, res_out).  Elementwise bound with 2K
    in place of K (the extra b*normw and t*bw product roundings, the
    sum-of-squares error and rsqrt all fit in the second K); res_out must be
    bit-equal.  ``fro_tol`` replaces the elementwise bound by a relative
    Frobenius bound (CPU fallback, which rounds t and y to bf16)."""
    for N in Ns:
        b = rand_bf16(gen, N, K)
        normw = rand_bf16(gen, K)
        for M in Ms:
            calls = ([onehot_x(c, K) for c in onehot_calls(M, K)] if onehot
                     else [rand_bf16(gen, M, K)])
            for x in calls:
                res = rand_bf16(gen, M, K) if with_res else None
                if onehot and with_res:
                    x = x * 0.5   # x + res is exactly one-hot
                    res = x.clone()
                c, res_out = fn(x.to(dev), res.to(dev) if res is not None else None,
                                normw.to(dev), b.to(dev), eps)
                c64, ro, absdot = gemv_norm_ref64(x, res, normw, b, eps)
                what = f"gemv_norm M={M} N={N} K={K} res={with_res} onehot={onehot}"
                assert_bits_equal(res_out, ro, what + " res_out")
                if fro_tol is not None:
                    assert rel_fro(c, c64) <= fro_tol, what
                else:
                    assert_within(c, c64, gemv_bound(c64, absdot, K, kfactor=2), what)


def check_swiglu_onehot(fn, Ns, K, dev, gen):
    """fn(gateup [1,2K], w [N,K]).  Activation == 32 e_k exactly, so the
    output is 32 W[:, k] bit for bit."""
    for N in Ns:
        w = rand_bf16(gen, N, K)
        wd = w.to(dev)
        for k in probe_columns(K):
            got = fn(swiglu_onehot_gateup(gen, k, K).to(dev), wd)
            exp = exact_bf16(32.0 * w[:, k].double()).unsqueeze(0)
            assert_bits_equal(got, exp, f"swiglu one-hot N={N} K={K} k={k}")


SWIGLU_FRO_TOL = 2.0 ** -8


def check_swiglu_random(fn, Ns, K, dev, gen):
    """The activation is rounded to bf16 before the dot, so the check is the
    relative Frobenius error: two independent bf16 roundings in quadrature
    give ~2e-3 (measured on MI355X: 1.8e-3 .. 2.6e-3, and up to 3.4e-3 at
    N=8 where only 8 outputs are averaged); a dropped 512-slot at K=5120
    gives ~0.3.  Bound 2^-8 = 3.9e-3."""
    for N in Ns:
        w = rand_bf16(gen, N, K)
        gu = rand_bf16(gen, 1, 2 * K)
        got = fn(gu.to(dev), w.to(dev))
        ref = swiglu_ref64(gu) @ w.double().t()
        r = rel_fro(got, ref)
        print(f"swiglu random N={N} K={K}: rel_fro={r:.3e}")
        assert r <= SWIGLU_FRO_TOL, f"swiglu random N={N} K={K}: rel_fro={r:.3e}"


def check_paged_onehot(fn, ctx, dev, gen, H=2, min_gap=60.0):
    """fn(q, kcache, vcache, block_table, ctx_lens, scale) -> [B,H,D]."""
    case = make_paged_case(gen, [ctx], H, H)
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in case.items()}
    for i, p in enumerate(probe_positions(ctx)):
        h = i % H
        kc, gap, v_row = plant_spike(case, 0, h, p)
        assert gap >= min_gap, f"generator: score gap {gap} < {min_gap}"
        got = fn(d["q"], kc.to(dev), d["vcache"], d["block_table"], d["ctx_lens"],
                 case["scale"])
        assert_bits_equal(got[0, h], v_row, f"paged one-hot ctx={ctx} p*={p} head={h}")


def check_paged_random(fn, ctxs, H, Hk, dev, gen, mode):
    """mode: 'diffuse' | 'peaked' (q x 4, outputs O(1)) | 'late_spike'
    (K[ctx-3] *= 8: alpha << 1 in a later pass and a rescale in the merge)."""
    case = make_paged_case(gen, ctxs, H, Hk, qscale=4.0 if mode == "peaked" else 1.0)
    if mode == "late_spike":
        P, _, _, D = case["kcache"].shape
        kflat = case["kcache"].view(P * PAGE, Hk, D)
        for b, ctx in enumerate(ctxs):
            if ctx >= 3:
                s = slots_of(case["block_table"][b], ctx)[ctx - 3]
                kflat[s] = (kflat[s].float() * 8).to(BF16)
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in case.items()}
    got = fn(d["q"], d["kcache"], d["vcache"], d["block_table"], d["ctx_lens"],
             case["scale"])
    ref = paged_decode_attn_ref64(case["q"], case["kcache"], case["vcache"],
                                  case["block_table"], case["ctx_lens"], case["scale"])
    assert_within(got, ref, torch.tensor(attn_bound(case["vcache"]), dtype=torch.float64),
                  f"paged random ctxs={ctxs} H={H} Hk={Hk} {mode}")


def check_rope_kv_append(fn, Hq, Hk, D, dev, gen, rope_tables, P=8, max_pos=300):
    """fn(qkv, cos_sin, positions, slot, kcache_flat, vcache_flat, Hq, Hk, D) -> q."""
    pos = torch.tensor([0, 1, 17, max_pos - 1, 0], dtype=torch.int32)
    slot = torch.tensor([0, P * PAGE - 1, 5, 21, 64], dtype=torch.int32)
    B = pos.numel()
    qs, kvs = Hq * D, Hk * D
    qkv = rand_bf16(gen, B, qs + 2 * kvs)
    cs = rope_tables(max_pos, D, 500000.0)
    kc = torch.full((P * PAGE, Hk, D), SENTINEL, dtype=BF16)
    vc = torch.full((P * PAGE, Hk, D), SENTINEL, dtype=BF16)
    kcd, vcd = kc.clone().to(dev), vc.clone().to(dev)  # .to() aliases on the CPU
    q = fn(qkv.to(dev), cs.to(dev), pos.to(dev), slot.to(dev), kcd, vcd, Hq, Hk, D)
    q_in = qkv[:, :qs].reshape(B, Hq, D)
    k_in = qkv[:, qs:qs + kvs].reshape(B, Hk, D)
    v_in = qkv[:, qs + kvs:].reshape(B, Hk, D)
    q64, qb = rope_ref64(q_in, cs, pos)
    k64, kb = rope_ref64(k_in, cs, pos)
    what = f"rope_kv_append Hq={Hq} Hk={Hk} D={D}"
    assert_within(q, q64, qb, what + " q")
    sl = slot.long()
    assert_within(kcd.cpu()[sl], k64, kb, what + " k")
    assert_bits_equal(vcd.cpu()[sl], v_in.contiguous(), what + " v rows")
    for i in (pos == 0).nonzero().flatten().tolist():   # cos = 1, sin = 0
        assert_bits_equal(q.cpu()[i], q_in[i].contiguous(), what + " q at position 0")
        assert_bits_equal(kcd.cpu()[sl[i]], k_in[i].contiguous(), what + " k at position 0")
    untouched = torch.ones(P * PAGE, dtype=torch.bool)
    untouched[sl] = False
    assert_bits_equal(kcd.cpu()[untouched], kc[untouched], what + " stray K-cache write")
    assert_bits_equal(vcd.cpu()[untouched], vc[untouched], what + " stray V-cache write")


def check_rope_scatter(fn, Hq, Hk, D, dev, gen, rope_tables, B=2, S=64, max_pos=300):
    """fn(qkv, cos_sin, positions, Hq, Hk, D, B, S) -> (q [B,Hq,S,D], k [B,Hk,S,D])."""
    T = B * S
    pos = torch.randint(0, max_pos, (T,), generator=gen).to(torch.int32)
    pos[0], pos[1], pos[T - 1] = 0, max_pos - 1, 0
    qs, kvs = Hq * D, Hk * D
    qkv = rand_bf16(gen, T, qs + 2 * kvs)
    cs = rope_tables(max_pos, D, 500000.0)
    qo, ko = fn(qkv.to(dev), cs.to(dev), pos.to(dev), Hq, Hk, D, B, S)
    q_in = qkv[:, :qs].reshape(T, Hq, D)
    k_in = qkv[:, qs:qs + kvs].reshape(T, Hk, D)
    what = f"rope_scatter Hq={Hq} Hk={Hk} D={D}"
    for got, x_in, Hh, nm in ((qo, q_in, Hq, "q"), (ko, k_in, Hk, "k")):
        assert tuple(got.shape) == (B, Hh, S, D)
        got_t = got.cpu().permute(0, 2, 1, 3).reshape(T, Hh, D)  # token-major
        r64, bnd = rope_ref64(x_in, cs, pos)
        assert_within(got_t, r64, bnd, f"{what} {nm}")
        z = (pos == 0).nonzero().flatten()
        assert_bits_equal(got_t[z].contiguous(), x_in[z].contiguous(),
                          f"{what} {nm} at position 0")


def check_argmax(fn, vocab, dev, gen, single_rows=False):
    """fn(logits [R, vocab] bf16) -> int32 [R]."""
    logits, names = argmax_edge_rows(gen, vocab)
    exp = argmax_ref_rows(logits)
    if single_rows:
        got = torch.cat([fn(logits[i:i + 1].contiguous().to(dev)).cpu()
                         for i in range(logits.shape[0])])
    else:
        got = fn(logits.to(dev)).cpu()
    assert got.dtype == torch.int32
    for i, nm in enumerate(names):
        g, e = int(got[i]), int(exp[i])
        assert 0 <= g < vocab, f"argmax vocab={vocab} {nm}: {g} out of range"
        assert g == e, f"argmax vocab={vocab} {nm}: got {g} expected {e}"
    fixed = {"max_first": 0, "max_last": vocab - 1, "all_equal": 0, "all_neg_inf": 0,
             "all_nan": 0, "nan_first_max_last": vocab - 1,
             "tie_across_passes": 8 * 255 + 3}
    for i, nm in enumerate(names):
        if nm in fixed:
            assert int(exp[i]) == fixed[nm], f"oracle: {nm}"


def check_target_logprob(fn, vocab, dev, gen, tol=1e-3):
    """fn(logits, targets) -> f32 [R]; atol = rtol = 1e-3, all finite."""
    logits, tgt, names = target_logprob_edge_rows(gen, vocab)
    got = fn(logits.to(dev), tgt.to(dev)).cpu().double()
    ref = target_logprob_ref64(logits, tgt)
    assert bool(torch.isfinite(ref).all()), "oracle: finite targets only"
    for i, nm in enumerate(names):
        g, r = float(got[i]), float(ref[i])
        assert math.isfinite(g), f"target_logprob vocab={vocab} {nm}: got {g} (ref {r})"
        assert abs(g - r) <= tol + tol * abs(r), \
            f"target_logprob vocab={vocab} {nm}: got {g} ref {r}"
    # a row with nothing finite has no distribution: NaN, as torch gives
    allneg = torch.full((1, vocab), float("-inf"), dtype=BF16)
    out = fn(allneg.to(dev), torch.zeros(1, dtype=torch.int32).to(dev))
    assert bool(torch.isnan(out).all())


# --------------------------------------------------------------------------
# Prefill attention (causal, GQA, D = 128).  The op under test is
# ``fn(q [B,H,S,D], k [B,Hk,S,D], vt [B,Hk,D,S], scale) -> O^T [B,H,D,S]``.
# --------------------------------------------------------------------------
PREFILL_D = 128
PREFILL_SCALE = 1.0 / math.sqrt(PREFILL_D)
V_FLOOR = 2.0 ** -6          # pointer cases: every |v| is at least this
POINTER_MIN_GAP = 60.0       # nats between the target and every other key
SCORE_LOG2_MAX = 300.0       # premise of prefill_bound: |score * log2 e|
PREFILL_S_MAX = 2048         # premise of prefill_bound
DEFER_THRESHOLD = 8.0        # nats; the kernels' documented defer-max rule
POINTER_MAPS = ("diag", "first", "tile_first", "tile_prev_last",
                "wave_prev_last", "random")
PREFILL_MODES = ("diffuse", "peaked", "early_spike",
                 "stair+3", "stair+7", "stair+9", "stair-7")


def kv_head_of(H: int, Hk: int) -> torch.Tensor:
    """Query head -> kv head (GQA: consecutive groups of H/Hk heads)."""
    assert H % Hk == 0
    return torch.arange(H) // (H // Hk)


def _scores64(q, k, scale, b, heads) -> torch.Tensor:
    """Unmasked fp64 scores [len(heads), S, S] of batch b."""
    kvh = kv_head_of(q.shape[1], k.shape[1])[heads]
    return (q[b, heads].double() @ k[b, kvh].double().transpose(-1, -2)) * scale


def attn_prefill_ref64(q, k, v, scale) -> torch.Tensor:
    """Causal GQA attention on the bf16 values as given, softmax in fp64.
    q [B,H,S,D], k/v [B,Hk,S,D] -> [B,H,S,D] fp64."""
    q, k, v = q.cpu(), k.cpu(), v.cpu()
    B, H, S, D = q.shape
    kvh = kv_head_of(H, k.shape[1])
    hidden = torch.ones(S, S, dtype=torch.bool).triu(1)   # key j > row i
    out = torch.empty(B, H, S, D, dtype=torch.float64)
    heads = torch.arange(H)
    for b in range(B):
        s = _scores64(q, k, scale, b, heads).masked_fill(hidden, float("-inf"))
        out[b] = torch.softmax(s, dim=-1) @ v[b, kvh].double()
    return out


def max_abs_score_log2(q, k, scale) -> float:
    """max |score| * log2(e) over ALL (row, key) pairs, masked ones included
    (the kernels compute a masked score before they discard it)."""
    q, k = q.cpu(), k.cpu()
    B, H = q.shape[:2]
    m = 0.0
    for b in range(B):
        for h0 in range(0, H, 64):
            heads = torch.arange(h0, min(H, h0 + 64))
            m = max(m, float(_scores64(q, k, scale, b, heads).abs().max()))
    return m * math.log2(math.e)


def prefill_bound(v: torch.Tensor) -> float:
    """(2^-8 + 2^-12) max|V|: elementwise bound on |kernel - fp64 reference|
    for |score * log2 e| <= 300 and S <= 2048 (both asserted by the checks).

    The kernels compute p_j = exp(s_j - m) in fp32, sum l = sum p_j from the
    UNROUNDED p_j, round p_j to bf16 for the PV MFMA, accumulate in fp32 and
    round o = (sum p_j v_j) / l to bf16.

    * 2^-9 max|V| for P rounded to bf16: each weight moves by a relative
      delta_j, the output by sum_j delta_j p_j v_j / l.  Half a bf16 ulp is
      between 2^-9 and 2^-8 of the value, so the strict worst case (every
      delta_j at its maximum, all with the sign of v_j, every |v_j| at
      max|V|) would be 2^-8 max|V|; the term used here holds once the
      delta_j are not all adversarial, which the measured ratios (printed
      per case) confirm.  A weight of exactly 1 (one dominating key) rounds
      without error.
    * 2^-9 |o| <= 2^-9 max|V| for the bf16 rounding of the output (|o| <=
      max|V|: a convex combination), with the same remark.
    * 2^-12 max|V| for the fp32 terms: the exponent's argument is off by at
      most 300 * 2^-23 relative (product and subtraction roundings at
      magnitude <= 300), the fp32 sums by S * 2^-24 <= 2^-13 relative, and
      v_exp_f32 / rcp by about an ulp each — together < 2^-12 relative.
    """
    return (2.0 ** -8 + 2.0 ** -12) * float(v.double().abs().max())


def clamp_v(v: torch.Tensor) -> torch.Tensor:
    """Every |v| pushed up to at least 2^-6 (sign kept, zero -> +2^-6): the
    pointer cases compare bits, and a zero element would let the e^-gap
    dust of the other keys decide its sign and value."""
    floor = torch.where(v < 0, -V_FLOOR, V_FLOOR).to(v.dtype)
    return torch.where(v.abs() < V_FLOOR, floor, v)


def pointer_targets(tmap: str, S: int, gen: torch.Generator) -> torch.Tensor:
    """Target key t(i) <= i for every row i (int64 [S])."""
    i = torch.arange(S)
    if tmap == "diag":
        t = i.clone()
    elif tmap == "first":
        t = torch.zeros(S, dtype=torch.int64)
    elif tmap == "tile_first":
        t = 64 * (i // 64)
    elif tmap == "tile_prev_last":
        t = (64 * (i // 64) - 1).clamp(min=0)
    elif tmap == "wave_prev_last":
        t = (32 * (i // 32) - 1).clamp(min=0)
    elif tmap == "random":
        t = (torch.rand(S, generator=gen, dtype=torch.float64) * (i + 1)).long()
        t = torch.minimum(t, i)
    else:
        raise ValueError(tmap)
    assert bool((t <= i).all()) and bool((t >= 0).all())
    return t


def _sign_codes(gen, *shape) -> torch.Tensor:
    return (torch.randint(0, 2, shape, generator=gen) * 2 - 1).to(BF16)


def make_pointer_case(gen, B, H, Hk, S, tmap) -> dict:
    """Pointer attention: K[j] = c_j in {+-1}^128, Q[i] = 16 c_t(i), codes and
    V drawn per (batch, kv head).  Every score is an exact integer times
    scale; the target scores 16 * 128 * scale = 181.02 nats.  ``expected`` is
    V[t(i)] per row, [B,H,S,D]."""
    D = PREFILL_D
    codes = _sign_codes(gen, B, Hk, S, D)
    t = pointer_targets(tmap, S, gen)
    kvh = kv_head_of(H, Hk)
    q = (codes[:, kvh][:, :, t].float() * 16.0).to(BF16)
    v = clamp_v(rand_bf16(gen, B, Hk, S, D))
    assert float(v.abs().min()) >= V_FLOOR
    if B * Hk > 1:   # a wrong batch / head index must land on other bits
        flat = v.reshape(B * Hk, -1)
        assert not any(torch.equal(flat[0], flat[i]) for i in range(1, B * Hk))
    return dict(q=q, k=codes, v=v, vt=v.transpose(-1, -2).contiguous(),
                scale=PREFILL_SCALE, t=t, expected=v[:, kvh][:, :, t].contiguous())


def pointer_min_gap(q, k, t, scale) -> float:
    """min over EVERY row of (score of the target - best other score), in
    fp64, the other keys taken over the whole sequence (not only the visible
    ones — the stricter reading)."""
    B, H, S, _ = q.shape
    idx = t.view(1, S, 1)
    gap = float("inf")
    for b in range(B):
        for h0 in range(0, H, 64):
            heads = torch.arange(h0, min(H, h0 + 64))
            s = _scores64(q, k, scale, b, heads)
            ix = idx.expand(len(heads), S, 1)
            tgt = s.gather(2, ix).squeeze(2)
            other = s.scatter(2, ix, float("-inf")).max(dim=2).values
            gap = min(gap, float((tgt - other).min()))
    return gap


def check_pointer(fn, B, H, Hk, S, tmap, dev, gen, prep=None):
    """Every row must return V[t(i)] BIT FOR BIT: the target's weight is
    exp(0) = 1, every other weight <= e^-60 (1e-26, against half an fp32 ulp
    of 6e-8), so l = 1, 1/l = 1 and the accumulated dust is < 2^-24 |v| for
    |v| >= 2^-6.  This holds across defer-max: before the target's tile the
    weights are <= e^8 relative to a stale max, and the rescale at the
    target multiplies them down to <= e^-gap.  ``prep`` maps the device q
    and k before the call (non-contiguous views)."""
    c = make_pointer_case(gen, B, H, Hk, S, tmap)
    gap = pointer_min_gap(c["q"], c["k"], c["t"], c["scale"])
    assert gap >= POINTER_MIN_GAP, f"generator: score gap {gap} < {POINTER_MIN_GAP}"
    q, k = c["q"].to(dev), c["k"].to(dev)
    if prep is not None:
        q, k = prep(q), prep(k)
    got = fn(q, k, c["vt"].to(dev), c["scale"])
    what = f"pointer {tmap} B={B} H={H} Hk={Hk} S={S}"
    assert tuple(got.shape) == (B, H, PREFILL_D, S), f"{what}: not O^T [B,H,D,S]"
    assert_bits_equal(got, c["expected"].transpose(-1, -2).contiguous(), what)
    return gap


def make_decoy_case(gen, B, H, Hk, S) -> dict:
    """Q[i] = 16 c_{i+1} for i < S-1 (the last row points at itself): the
    strongest key of every row is the first MASKED one."""
    c = make_pointer_case(gen, B, H, Hk, S, "diag")
    t = torch.arange(S)
    t[:-1] += 1
    kvh = kv_head_of(H, Hk)
    c["q"] = (c["k"][:, kvh][:, :, t].float() * 16.0).to(BF16)
    c["t"] = t
    del c["expected"]
    return c


def check_future_decoy(fn, B, H, Hk, S, dev, gen):
    """The mask must hide a key that would dominate.  Expectation: the fp64
    softmax over keys <= i within prefill_bound; row 0 == V[0] bit for bit.
    Premises, every row: the decoy beats every visible key by >= 60 nats,
    and (rows 1 .. S-2) the reference is further than 4 bounds from V[i+1]
    in at least one element, so a leak cannot pass."""
    c = make_decoy_case(gen, B, H, Hk, S)
    q, k, v = c["q"], c["k"], c["v"]
    kvh = kv_head_of(H, Hk)
    assert S <= PREFILL_S_MAX and max_abs_score_log2(q, k, c["scale"]) <= SCORE_LOG2_MAX
    hidden = torch.ones(S, S, dtype=torch.bool).triu(1)
    for b in range(B):
        s = _scores64(q, k, c["scale"], b, torch.arange(H))
        decoy = s.diagonal(offset=1, dim1=1, dim2=2)                  # [H, S-1]
        vis = s.masked_fill(hidden, float("-inf")).max(dim=2).values  # [H, S]
        lead = float((decoy - vis[:, :-1]).min())
        assert lead >= POINTER_MIN_GAP, f"generator: decoy leads by only {lead}"
    ref = attn_prefill_ref64(q, k, v, c["scale"])
    bound = prefill_bound(v)
    leak = v[:, kvh].double()[:, :, 2:]                               # V[i+1], i = 1..S-2
    sep = (ref[:, :, 1:S - 1] - leak).abs().max(dim=-1).values
    assert float(sep.min()) > 4 * bound, "generator: a leak would pass"
    got = fn(q.to(dev), k.to(dev), c["vt"].to(dev), c["scale"])
    what = f"future decoy B={B} H={H} Hk={Hk} S={S}"
    assert tuple(got.shape) == (B, H, PREFILL_D, S), f"{what}: not O^T [B,H,D,S]"
    ratio = err_ratio(got, ref.transpose(-1, -2), bound)
    print(f"{what}: max err / bound = {ratio:.3f}")
    assert_within(got, ref.transpose(-1, -2), bound, what)
    assert_bits_equal(got[:, :, :, 0], v[:, kvh][:, :, 0], what + " row 0")
    return ratio


def err_ratio(got, ref64, bound: float) -> float:
    return float((got.detach().cpu().double() - ref64).abs().max()) / bound


def make_prefill_case(gen, mode, B, H, Hk, S) -> dict:
    """Random / staircase inputs.  'diffuse': randn.  'peaked': q x 4.
    'early_spike': K[100] x 8.  'stair<step>': Q[i] = u (one sign vector per
    (batch, kv head)), K[j] = kappa_j u + randn with kappa_j =
    bf16(step * (j // 64) / sqrt(128)), so the scores climb (or fall) by
    ``step`` nats per 64-key tile with N(0,1) noise on top."""
    D = PREFILL_D
    kvh = kv_head_of(H, Hk)
    v = rand_bf16(gen, B, Hk, S, D)
    if mode.startswith("stair"):
        step = float(mode[len("stair"):])
        u = _sign_codes(gen, B, Hk, 1, D)
        q = u[:, kvh].expand(B, H, S, D).contiguous()
        kappa = (step * (torch.arange(S) // 64).double() / math.sqrt(D)).to(BF16)
        k = (kappa.float().view(1, 1, S, 1) * u.float()
             + torch.randn(B, Hk, S, D, generator=gen)).to(BF16)
    else:
        q = torch.randn(B, H, S, D, generator=gen)
        q = (q * 4.0 if mode == "peaked" else q).to(BF16)
        k = rand_bf16(gen, B, Hk, S, D)
        if mode == "early_spike":
            assert S > 100
            k[:, :, 100] = (k[:, :, 100].float() * 8.0).to(BF16)
        assert mode in ("diffuse", "peaked", "early_spike"), mode
    return dict(q=q, k=k, v=v, vt=v.transpose(-1, -2).contiguous(), scale=PREFILL_SCALE)


def stair_tile_maxes(q, k, scale, b=0, h=0) -> torch.Tensor:
    """fp64 max score of each 64-key tile as the LAST row sees it (all keys
    visible; every row of a staircase case has the same q)."""
    s = _scores64(q, k, scale, b, torch.tensor([h]))[0, -1]
    return s.view(-1, 64).max(dim=1).values


def defer_pattern(tile_max: torch.Tensor, thr: float = DEFER_THRESHOLD) -> str:
    """The defer-max rule replayed in fp64 on a row's tile maxima: 'D' where
    a tile stays within ``thr`` nats of the running max (max kept stale),
    'R' where it rescales.  The first tile always rescales (from -inf)."""
    m, out = float("-inf"), []
    for t in tile_max.tolist():
        if t - m <= thr:
            out.append("D")
        else:
            out.append("R")
            m = max(m, t)
    return "".join(out)


def assert_stair_premises(q, k, scale, mode):
    """Measured in fp64 for every (batch, head): the mean step per tile is
    within 1 nat of the nominal one and every single step within 2.5 (the
    max of 64 N(0,1) draws has a standard deviation of about 0.5, a step is
    the difference of two, the mean step (M_last - M_0) / (tiles - 1));
    the defer rule then goes through the regime the case is meant for."""
    step = float(mode[len("stair"):])
    B, H = q.shape[:2]
    for b in range(B):
        for h in range(H):
            M = stair_tile_maxes(q, k, scale, b, h)
            d = M[1:] - M[:-1]
            assert abs(float(d.mean()) - step) <= 1.0, f"{mode}: mean step {float(d.mean())}"
            assert float((d - step).abs().max()) <= 2.5, f"{mode}: steps {d.tolist()}"
            pat = defer_pattern(M)[1:]
            if step == 3:      # defer, defer, rescale: each under 8, the sum over
                # (three tiles, S = 192, end before the rescale)
                assert "DDR" in pat if len(pat) >= 3 else pat == "DD", pat
            elif step == 7:    # defer and rescale alternate; never two defers
                assert "DR" in pat and "DD" not in pat, pat
                assert len(pat) < 3 or "RD" in pat, pat
            elif step == 9:    # rescales back to back (a step that the noise
                # brings under 8 still defers now and then, never twice)
                assert "DD" not in pat and pat.count("R") >= pat.count("D"), pat
                assert len(pat) < 4 or "RR" in pat, pat
            elif step == -7:   # every tile defers against tile 0's max
                assert pat == "D" * len(pat), pat
            else:
                raise ValueError(mode)


def check_prefill_random(fn, mode, B, H, Hk, S, dev, gen):
    """fn against attn_prefill_ref64 within prefill_bound, elementwise; row 0
    (one visible key: p = 1, l = 1) must equal V[0] bit for bit.  Returns the
    measured max error / bound (also printed)."""
    c = make_prefill_case(gen, mode, B, H, Hk, S)
    q, k, v = c["q"], c["k"], c["v"]
    assert S <= PREFILL_S_MAX
    smax = max_abs_score_log2(q, k, c["scale"])
    assert smax <= SCORE_LOG2_MAX, f"generator: |score log2 e| = {smax}"
    if mode.startswith("stair"):
        assert_stair_premises(q, k, c["scale"], mode)
    ref = attn_prefill_ref64(q, k, v, c["scale"]).transpose(-1, -2)
    bound = prefill_bound(v)
    got = fn(q.to(dev), k.to(dev), c["vt"].to(dev), c["scale"])
    what = f"prefill {mode} B={B} H={H} Hk={Hk} S={S}"
    assert tuple(got.shape) == (B, H, PREFILL_D, S), f"{what}: not O^T [B,H,D,S]"
    ratio = err_ratio(got, ref, bound)
    print(f"{what}: max err / bound = {ratio:.3f}")
    assert_within(got, ref, bound, what)
    assert_bits_equal(got[:, :, :, 0], v[:, kv_head_of(H, Hk)][:, :, 0], what + " row 0")
    return ratio


def check_vt_from_qkv(fn, B, S, Hq, Hk, D, dev, gen, extra_cols=0):
    """fn(qkv [B*S, (Hq+2Hk)*D + extra_cols], Hq, Hk, D, B, S) -> V^T
    [B,Hk,D,S], a pure copy: bit-equal to permute(0,2,3,1).contiguous()."""
    ld = (Hq + 2 * Hk) * D + extra_cols
    qkv = rand_bf16(gen, B * S, ld)
    exp = qkv[:, (Hq + Hk) * D:(Hq + 2 * Hk) * D].reshape(B, S, Hk, D)
    exp = exp.permute(0, 2, 3, 1).contiguous()
    got = fn(qkv.to(dev), Hq, Hk, D, B, S)
    assert_bits_equal(got, exp, f"vt_from_qkv B={B} S={S} Hq={Hq} Hk={Hk} D={D} ld={ld}")


# --------------------------------------------------------------------------
# Tiled quantized GEMM (e4m3 x e4m3: fp8 row scales / MX e8m0 block scales).
# The op under test is ``fn(a_q [M,K] u8, a_s, b_q [N,K] u8, b_s) -> C [M,N]
# bf16`` with a_s / b_s f32 [rows] (kind 'fp8') or u8 [rows, K/32] ('mx').
# --------------------------------------------------------------------------
QGEMM_KFACTOR = {"fp8": 32, "mx": 64}   # measured, see check_qgemm_random


def assert_bytes_equal(got: torch.Tensor, exp: torch.Tensor, what: str = ""):
    assert got.dtype == torch.uint8 and exp.dtype == torch.uint8, what
    assert got.shape == exp.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(exp.shape)}"
    g = got.detach().cpu()
    if torch.equal(g, exp):
        return
    bad = (g != exp).nonzero()
    i = tuple(int(v) for v in bad[0])
    raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} bytes differ; first at {i}: "
                         f"got 0x{int(g[i]):02x} expected 0x{int(exp[i]):02x}")


def qgemm_probe_columns(K: int) -> list:
    """probe_columns(K) plus both sides of every 16 / 32 / 64 / 128 boundary
    (16-byte LDS chunk, scale block, MFMA step, K-tile) and K - 1."""
    cols = set(probe_columns(K)) | {0, K - 1}
    for step in (16, 32, 64, 128):
        for b in range(step, K, step):
            cols.update((b - 1, b))
    return sorted(c for c in cols if 0 <= c < K)


def qgemm_onehot_cols(M: int, K: int) -> torch.Tensor:
    """Row m probes column cols[m % len(cols)]."""
    cols = qgemm_probe_columns(K)
    return torch.tensor([cols[m % len(cols)] for m in range(M)])


def mx_probe_scales(gen, M: int, N: int, nblk: int):
    """e8m0 bytes (A [M, nblk], B [N, nblk]) for the one-hot probe.  Within
    a row every block has another exponent (a random injection of the blocks
    into R = max(nblk, 8) slots); A's exponents are even, B's odd, so no A
    row equals any B row in any block.  One A row is lifted by +40 and one B
    row lowered by 40 (bytes near 167 / 87).  |exponent| <= R + 40 per side;
    with e4m3 products in 2^-18 .. 2^18 the outputs stay within 2^+-122."""
    assert nblk <= 32
    R = max(nblk, 8)

    def perms(rows):
        return torch.rand(rows, R, generator=gen).argsort(dim=1)[:, :nblk]

    ea = 2 * perms(M) - R
    eb = 2 * perms(N) - R + 1
    ea[min(1, M - 1)] += 40
    eb[min(2, N - 1)] -= 40
    return (ea + 127).to(torch.uint8), (eb + 127).to(torch.uint8)


def make_qgemm_case(kind: str, mode: str, gen, M: int, N: int, K: int):
    """mode 'onehot' | 'int' | 'random'.  Returns ((a_q, a_s, b_q, b_s),
    a64 [M,K], b64 [N,K]) with a64 / b64 the dequantized operands."""
    assert kind in ("fp8", "mx") and K % 32 == 0
    nblk = K // 32

    def pow2_rows(rows):
        return torch.exp2(torch.randint(-3, 4, (rows,), generator=gen).float())

    if mode == "onehot":
        a_q = torch.zeros(M, K, dtype=torch.uint8)
        a_q[torch.arange(M), qgemm_onehot_cols(M, K)] = _rand_e4m3_bytes(gen, M, 1)[:, 0]
        b_q = _rand_e4m3_bytes(gen, N, K)
        if kind == "fp8":
            a_s, b_s = pow2_rows(M), pow2_rows(N)
        else:
            a_s, b_s = mx_probe_scales(gen, M, N, nblk)
    elif mode == "int":
        a_q, b_q = _int_e4m3_bytes(gen, M, K), _int_e4m3_bytes(gen, N, K)
        if kind == "fp8":
            a_s, b_s = pow2_rows(M), pow2_rows(N)
        else:   # 2^-2 .. 2^2 per block: every product is a multiple of 2^-4
            a_s = torch.randint(125, 130, (M, nblk), generator=gen).to(torch.uint8)
            b_s = torch.randint(125, 130, (N, nblk), generator=gen).to(torch.uint8)
    elif mode == "random":
        a_q, b_q = _rand_e4m3_bytes(gen, M, K), _rand_e4m3_bytes(gen, N, K)
        if kind == "fp8":
            a_s = ((2.0 ** -4) * (1.0 + torch.rand(M, generator=gen))).float()
            b_s = ((2.0 ** -4) * (1.0 + torch.rand(N, generator=gen))).float()
        else:   # random e8m0 over +-6
            a_s = torch.randint(121, 134, (M, nblk), generator=gen).to(torch.uint8)
            b_s = torch.randint(121, 134, (N, nblk), generator=gen).to(torch.uint8)
    else:
        raise ValueError(mode)
    deq = dequant_fp8_ref64 if kind == "fp8" else dequant_mx_ref64
    return (a_q, a_s, b_q, b_s), deq(a_q, a_s), deq(b_q, b_s)


def qgemm_int_premise(kind, args, a64, b64) -> float:
    """Largest sum of |products| in units of the smallest product quantum;
    below 2^24 every partial sum, in any order, is exact in fp32.  fp8: the
    accumulator holds the UNSCALED integer sum (scales are applied after);
    mx: scaled products are multiples of 2^-4."""
    if kind == "fp8":
        a, b = e4m3_to_f64(args[0]), e4m3_to_f64(args[2])
        return float((a.abs() @ b.abs().t()).max())
    return float((a64.abs() @ b64.abs().t()).max()) * 16


def check_qgemm_onehot(fn, kind, M, N, K, dev, gen):
    """Row m of A_q has one non-zero byte, at a probe column; scales are
    powers of two (mx: another exponent for every (row, block)).  a * b has
    at most 8 significant bits, so C[m, n] = a b 2^(..) is a bf16 value and
    must come out bit for bit, for every m and n.  For kind 'mx' this pins
    the scale byte <-> K block mapping of both operands."""
    args, a64, b64 = make_qgemm_case(kind, "onehot", gen, M, N, K)
    ref = a64 @ b64.t()
    exp = exact_bf16(ref)
    assert torch.equal(exp.double(), ref), "generator: expectation is not a bf16 value"
    got = fn(*_to(dev, args))
    assert_bits_equal(got, exp, f"{kind} qgemm one-hot M={M} N={N} K={K}")


def check_qgemm_int(fn, kind, M, N, K, dev, gen):
    """Small integers over all of K with power-of-two scales: every partial
    sum is exact in fp32, so C == bf16_rne(exact sum) bit for bit.  Catches
    a dropped or doubled K-tile, a wrong swizzle or buffer parity and a hole
    in the workgroup remap."""
    args, a64, b64 = make_qgemm_case(kind, "int", gen, M, N, K)
    assert qgemm_int_premise(kind, args, a64, b64) < 2 ** 24
    exp = exact_bf16(a64 @ b64.t())
    got = fn(*_to(dev, args))
    assert_bits_equal(got, exp, f"{kind} qgemm integer M={M} N={N} K={K}")


def check_qgemm_random(fn, kind, M, N, K, dev, gen, kfactor=None):
    """Random finite bytes, non-power-of-two f32 row scales (fp8) / random
    e8m0 over +-6 (mx).  Elementwise bound: gemv_bound(ref, |A|.|B|^T, K,
    kfactor) — bf16 output rounding plus worst-case fp32 summation in any
    order (e4m3 x e4m3 products are exact) — plus 2 * 2^-24 |ref| for the fp8
    epilogue's two f32 multiplies.

    kfactor = 1 does not hold on the MI355X: the fp8 MFMAs do not add their
    32 / 64 products as separately rounded fp32 terms (the error pattern is
    that of small products losing bits against the largest one of the
    instruction — random e4m3 bytes span 2^36 in the products; integer and
    one-hot data stay bit-exact).  Measured against this fp64 reference on every
    (M, N, K) of tests/test_quant_gemm_edges_gpu.py, three draws each, the
    worst err / bound at kfactor = 1 was 12.2 for fp8 (at K = 128; 1.3 at
    K = 640) and 19.3 for mx (at 2560 x 4352 x 128; 13.3 at the shapes the
    random tests run).  The excess is about 1000 .. 3400 x 2^-24 |A|.|B|^T
    whatever K is.  QGEMM_KFACTOR is the smallest power of two that leaves a
    2x margin over those ratios: 32 for fp8, 64 for mx.  The CPU fallbacks
    (true fp32 sums) stay below 1.0 at kfactor = 1.
    Returns (and prints) the worst err / bound."""
    args, a64, b64 = make_qgemm_case(kind, "random", gen, M, N, K)
    ref = a64 @ b64.t()
    absdot = a64.abs() @ b64.abs().t()
    bound = gemv_bound(ref, absdot, K, QGEMM_KFACTOR[kind] if kfactor is None else kfactor)
    if kind == "fp8":
        bound = bound + 2 * U_FP32 * ref.abs()
    got = fn(*_to(dev, args))
    what = f"{kind} qgemm random M={M} N={N} K={K}"
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)}"
    err = (got.detach().cpu().double() - ref).abs()
    ratio = float((err / bound).max())
    # the summation term on its own: error left after a full bf16 half-ulp
    excess = float(((err - U_BF16_OUT * ref.abs()) / (K * U_FP32 * absdot)).max())
    print(f"{what}: max err / bound = {ratio:.3f}; "
          f"max (err - 2^-8|ref|) / (K 2^-24 |A|.|B|) = {excess:.3f}")
    assert_within(got, ref, bound, what)
    return ratio


# --------------------------------------------------------------------------
# Grouped GEMM (MoE).  ``fn(a_sorted [T,K] bf16, w [E,N,K] bf16, seg) -> C``
# with seg a host list of E+1 offsets or a device int32 tensor of E ends.
# --------------------------------------------------------------------------
def make_grouped_case(gen, sizes, N, K, mode):
    """Expert-sorted activations and per-expert weights that differ from
    every other expert's in EVERY element.  mode 'int': A in [-2, 2],
    W[e] = ((base + e) mod 9) - 4; 'random': A randn, W[e] = r 2^(e - E/2)
    with one shared non-zero r.  Returns (a, w, starts, ref64, absdot)."""
    E, T = len(sizes), sum(sizes)
    assert 1 <= E <= 9
    if mode == "int":
        a = int_x(gen, T, K)
        base = torch.randint(0, 9, (N, K), generator=gen)
        w = torch.stack([((base + e) % 9) - 4 for e in range(E)]).to(BF16)
    elif mode == "random":
        a = rand_bf16(gen, T, K)
        r = clamp_v(rand_bf16(gen, N, K))
        w = torch.stack([(r.float() * 2.0 ** (e - E // 2)).to(BF16) for e in range(E)])
    else:
        raise ValueError(mode)
    for e in range(E):
        for f in range(e + 1, E):
            assert bool((w[e] != w[f]).all()), "generator: experts share an element"
    starts = [0]
    for s in sizes:
        starts.append(starts[-1] + s)
    ref = torch.zeros(T, N, dtype=torch.float64)
    absdot = torch.zeros(T, N, dtype=torch.float64)
    for e in range(E):
        s, t = starts[e], starts[e + 1]
        ref[s:t] = a[s:t].double() @ w[e].double().t()
        absdot[s:t] = a[s:t].double().abs() @ w[e].double().abs().t()
    return a, w, starts, ref, absdot


def check_grouped_gemm(fn, sizes, N, K, dev, gen, offsets="host"):
    """Every row of every segment (so both sides of each segment end): bit
    for bit on integer data, within the bf16 GEMV bound on random data.
    ``a_sorted`` is passed with exactly sum(sizes) rows — no spare rows."""
    T = sum(sizes)
    for mode in ("int", "random"):
        a, w, starts, ref, absdot = make_grouped_case(gen, sizes, N, K, mode)
        if offsets == "host":
            seg = list(starts)
        else:
            seg = torch.tensor(starts[1:], dtype=torch.int32).to(dev)
        got = fn(a.to(dev), w.to(dev), seg)
        what = f"grouped gemm {mode} sizes={sizes} N={N} K={K} offsets={offsets}"
        assert got.dim() == 2 and got.shape[0] >= T and got.shape[1] == N, \
            f"{what}: shape {tuple(got.shape)}"
        got = got[:T]
        if mode == "int":
            assert float(absdot.max()) < 2 ** 24
            assert_bits_equal(got.contiguous(), exact_bf16(ref), what)
        else:
            assert_within(got, ref, gemv_bound(ref, absdot, K), what)


# --------------------------------------------------------------------------
# Quantizers
# --------------------------------------------------------------------------
E4M3_MAX = 448.0


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e in fp64 for integer e (exact)."""
    return torch.pow(torch.full((), 2.0, dtype=torch.float64), e.double())


def _e4m3_quantum(a: torch.Tensor) -> torch.Tensor:
    """Spacing of e4m3 values at magnitude a (fp64, a >= 0): 2^(e-3) with
    e = max(floor(log2 a), -6); 2^-9 in the subnormal range and at 0."""
    _, ex = torch.frexp(a)
    e = torch.where(a > 0, ex.long() - 1, torch.full_like(ex.long(), -6)).clamp(min=-6)
    return _pow2(e - 3)


def _e4m3_encode(val: torch.Tensor, neg: torch.Tensor) -> torch.Tensor:
    """Bytes of non-negative fp64 values that ARE e4m3 values, sign bit from
    ``neg``."""
    b = val.float().to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(e4m3_to_f64(b), val), "not an e4m3 value"
    return b | (neg.to(torch.uint8) << 7)


def e4m3_rne_bytes(v64: torch.Tensor) -> torch.Tensor:
    """Round-to-nearest-even of fp64 values to e4m3fn bytes, saturating at
    448; the sign bit is kept on a zero result.  Written out (not torch's
    conversion) so the expectation has one rounding, from the exact value."""
    a = v64.abs().clamp(max=E4M3_MAX)
    qn = _e4m3_quantum(a)
    return _e4m3_encode(torch.round(a / qn) * qn, torch.signbit(v64))   # round: half to even


def e4m3_neighbours(a: torch.Tensor):
    """(lo, hi): the e4m3 magnitudes around a >= 0; lo == a when a is one."""
    qn = _e4m3_quantum(a)
    lo = torch.floor(a / qn) * qn
    return lo, lo + qn


def all_e4m3_magnitudes() -> torch.Tensor:
    """The 127 finite e4m3fn magnitudes, ascending (0 .. 448)."""
    return e4m3_to_f64(torch.arange(0, 0x7f, dtype=torch.uint8))


def _bf16_step(v: float, up: bool) -> float:
    """The bf16 value one ulp above / below a positive bf16 value."""
    t = torch.tensor([v], dtype=BF16)
    assert float(t) == v and v > 0
    return float((t.view(torch.int16) + (1 if up else -1)).view(BF16))


def _fill(gen, amax: float, n: int, frac: float = 0.5) -> torch.Tensor:
    """n bf16 values of magnitude <= frac * amax."""
    u = torch.rand(n, generator=gen, dtype=torch.float64) * 2 - 1
    return (u * frac * amax).to(BF16)


def _midpoint_block() -> torch.Tensor:
    """32 values at scale 1 (amax 256 -> e = 0): exact e4m3 midpoints of
    every spacing down to the subnormals, both signs; ties go to even."""
    mids = [17, 19, 21, 23, 34, 38, 68, 76, 136, 152, 1.0625, 1.1875, 2.125, 2.375,
            0.5 * 2 ** -9, 1.5 * 2 ** -9, 2.5 * 2 ** -9, 4.5 * 2 ** -9, 7.5 * 2 ** -9,
            2.0 ** -6 + 2.0 ** -10]
    vals = [256.0] + mids + [-m for m in mids[:11]]
    assert len(vals) == 32
    return torch.tensor(vals, dtype=torch.float64)


def mx_special_blocks(gen) -> list:
    """(name, 32 bf16 values) blocks for quant_mxfp8's edges."""
    out = []

    def planted(name, amax, pos=0, neg=False, frac=0.5):
        b = _fill(gen, amax, 32, frac)
        b[pos] = -amax if neg else amax
        assert float(b[pos].double().abs()) == amax, f"{name}: amax is not a bf16 value"
        out.append((name, b))

    for j in (-20, 0, 9, 30):
        edge = 0.875 * 2.0 ** j      # m == 0.875: amax 2^-e == 448, no step
        planted(f"0.875*2^{j}", edge, pos=5)
        planted(f"0.875*2^{j}+ulp", _bf16_step(edge, True), pos=31, neg=True)
        planted(f"0.875*2^{j}-ulp", _bf16_step(edge, False), pos=0)
        planted(f"2^{j}", 2.0 ** j, pos=17)
        planted(f"2^{j}-ulp", _bf16_step(2.0 ** j, False), pos=16, neg=True)
    unit = 2.0 ** -133               # bf16 subnormal spacing
    b = (torch.randint(-3, 4, (32,), generator=gen).double() * unit).to(BF16)
    b[9] = 5 * unit
    out.append(("subnormal", b))
    b = (torch.randint(-100, 101, (32,), generator=gen).double() * 2.0 ** -140)
    b = b.to(BF16)                   # rounds to multiples of 2^-133, mostly 0
    b[3] = -unit
    out.append(("smallest subnormal", b))
    planted("bf16 max", float(torch.finfo(BF16).max), pos=30, frac=2.0 ** -7)
    planted("bf16 max, full block", float(torch.finfo(BF16).max), pos=1, neg=True, frac=1.0)
    out.append(("zero block", torch.zeros(32, dtype=BF16)))
    for p in range(32):
        planted(f"amax at {p}", 3.5 * 2.0 ** (p - 16), pos=p, neg=bool(p & 1), frac=0.25)
    for j in (0, -9, 13):
        b = (_midpoint_block() * 2.0 ** j).to(BF16)
        assert torch.equal(b.double(), _midpoint_block() * 2.0 ** j)
        out.append((f"midpoints*2^{j}", b))
    return out


def mx_quant_inputs(gen, rows: int, K: int) -> list:
    """Inputs [rows, K] bf16 for quant_mxfp8: random blocks spanning 2^+-30
    per block, every special block planted once (over as many calls as the
    shape needs), and row 1 all zero when there are at least three rows."""
    nblk = K // 32
    specials = mx_special_blocks(gen)
    zero_row = 1 if rows >= 3 else None
    free = [(r, b) for r in range(rows) if r != zero_row for b in range(nblk)]
    calls = []
    for c0 in range(0, len(specials), len(free)):
        x = torch.randn(rows, nblk, 32, generator=gen, dtype=torch.float64)
        x = (x * _pow2(torch.randint(-30, 31, (rows, nblk, 1), generator=gen))).to(BF16)
        perm = torch.randperm(len(free), generator=gen).tolist()
        for i, (_, blk) in enumerate(specials[c0:c0 + len(free)]):
            r, b = free[perm[i]]
            x[r, b] = blk
        if zero_row is not None:
            x[zero_row] = 0
        calls.append(x.reshape(rows, K))
    return calls


def quant_mxfp8_expect(x: torch.Tensor):
    """(q bytes [rows, K], scale bytes [rows, K/32]) by the fp64 rule:
    e = floor(log2 amax) - 8, + 1 if amax 2^-e > 448, clamped to [-127, 127];
    a zero block has byte 0.  The scale is a power of two, so x 2^-e is exact
    and q = RNE_e4m3 of the exact quotient."""
    rows, K = x.shape
    blk = x.cpu().double().view(rows, K // 32, 32)
    amax = blk.abs().amax(dim=-1)
    _, ex = torch.frexp(amax)
    e = ex.long() - 1 - 8
    e = e + (amax * _pow2(-e) > E4M3_MAX).long()
    e = torch.where(amax > 0, e, torch.full_like(e, -127)).clamp(-127, 127)
    quot = blk * _pow2(-e).unsqueeze(-1)
    assert float(quot.abs().max()) <= E4M3_MAX
    return e4m3_rne_bytes(quot).reshape(rows, K), (e + 127).to(torch.uint8)


def check_quant_mxfp8(fn, rows, K, dev, gen):
    """fn(x [rows, K] bf16) -> (q u8 [rows, K], s u8 [rows, K/32]): scale
    bytes and payload bytes EQUAL to quant_mxfp8_expect."""
    for c, x in enumerate(mx_quant_inputs(gen, rows, K)):
        q, s = fn(x.to(dev))
        q_exp, s_exp = quant_mxfp8_expect(x)
        what = f"quant_mxfp8 rows={rows} K={K} call {c}"
        assert_bytes_equal(s, s_exp, what + " scale")
        assert_bytes_equal(q, q_exp, what + " payload")


FP8_TIE_MARGIN = 4 * U_FP32   # two f32 roundings (1/s and x * (1/s)), relative
FP8_TIE_CAP = 1e-3            # share of a call's elements that may sit that close


def fp8_amax_positions(K: int) -> list:
    """Where the row maximum is planted: first / last element, the first and
    last element of each wave's share of the first pass (thread t takes
    vector t, so wave w covers elements [512 w, 512 w + 512)), and the
    vectors past 256 (thread 0's second pass: element 2048 at K = 2056)."""
    cand = [0, K - 1, K - 8]
    for w in range(4):
        cand += [512 * w, 512 * w + 511]
    cand += [2048, 2055]
    return sorted({p for p in cand if 0 <= p < K})


def _fp8_random_row(gen, K: int, pos=None) -> torch.Tensor:
    """randn clipped to +-3.9, the maximum (1 + odd/128) * 4 in [4, 8)
    planted at ``pos`` (odd significand: x 448 / amax never lands exactly
    on an e4m3 midpoint), all times 2^j."""
    r = torch.randn(K, generator=gen, dtype=torch.float64).clamp(-3.9, 3.9)
    odd = 2 * int(torch.randint(0, 64, (1,), generator=gen)) + 1
    if pos is None:
        pos = int(torch.randint(0, K, (1,), generator=gen))
    sign = -1.0 if int(torch.randint(0, 2, (1,), generator=gen)) else 1.0
    r[pos] = sign * (1 + odd / 128) * 4
    j = int(torch.randint(-10, 11, (1,), generator=gen))
    return (r * 2.0 ** j).to(BF16)


def _fp8_exact_row(gen, K: int, j: int) -> torch.Tensor:
    """amax = 448 * 2^j (scale 2^j and its inverse exact); every element an
    e4m3 value or the exact midpoint of two neighbours, times 2^j."""
    v = all_e4m3_magnitudes()
    pool = torch.cat([v, (v[:-1] + v[1:]) / 2])
    r = pool[torch.randint(0, pool.numel(), (K,), generator=gen)]
    r = r * (torch.randint(0, 2, (K,), generator=gen).double() * 2 - 1)
    r[int(torch.randint(0, K, (1,), generator=gen))] = E4M3_MAX
    row = (r * 2.0 ** j).to(BF16)
    assert torch.equal(row.double(), r * 2.0 ** j), "generator: not bf16 values"
    return row


def fp8_near_midpoint(x: torch.Tensor, s_ref: torch.Tensor) -> torch.Tensor:
    """Elements whose x / s lies within FP8_TIE_MARGIN (relative) of the
    midpoint of its two e4m3 neighbours (bool [rows, K])."""
    a = (x.cpu().double() / s_ref.double().unsqueeze(1)).abs().clamp(max=E4M3_MAX)
    lo, hi = e4m3_neighbours(a)
    mid = (lo + hi) / 2
    return (a - mid).abs() <= FP8_TIE_MARGIN * mid


def quant_fp8_scale_ref(x: torch.Tensor) -> torch.Tensor:
    """f32 amax / 448 (one correctly rounded division); 1 for a zero row."""
    amax = x.cpu().float().abs().amax(dim=-1)
    return torch.where(amax > 0, amax / torch.tensor(448.0), torch.ones_like(amax))


def fp8_quant_inputs(gen, rows: int, K: int) -> list:
    """[(x [rows, K] bf16, exact [rows] bool)]: amax planted at every
    fp8_amax_positions(K), exact rows (amax 448 * 2^j), a zero row and random
    rows, over as many calls as the shape needs.  Outside the exact rows at
    most FP8_TIE_CAP of a call's elements lie near a midpoint (a call is
    redrawn until that holds — the premise of the nearest-neighbour rule)."""
    recipes = [("pos", p) for p in fp8_amax_positions(K)]
    recipes += [("exact", j) for j in (-3, 0, 5)] + [("zero", None)]
    recipes += [("random", None)] * 4
    while len(recipes) % rows:
        recipes.append(("random", None))
    calls = []
    for c0 in range(0, len(recipes), rows):
        for _ in range(20):
            xs, exact = [], []
            for kind, arg in recipes[c0:c0 + rows]:
                exact.append(kind == "exact")
                if kind == "pos":
                    xs.append(_fp8_random_row(gen, K, arg))
                elif kind == "exact":
                    xs.append(_fp8_exact_row(gen, K, arg))
                elif kind == "zero":
                    xs.append(torch.zeros(K, dtype=BF16))
                else:
                    xs.append(_fp8_random_row(gen, K))
            x, exact = torch.stack(xs), torch.tensor(exact)
            near = fp8_near_midpoint(x, quant_fp8_scale_ref(x))[~exact]
            if int(near.sum()) <= int(FP8_TIE_CAP * x.numel()):
                break
        else:
            raise AssertionError("generator: too many elements near a midpoint")
        calls.append((x, exact))
    return calls


def judge_quant_fp8(x, exact, q, s, what="quant_fp8"):
    """The contract of check_quant_fp8 on one call's result (CPU tensors)."""
    x, q, s = x.cpu(), q.detach().cpu(), s.detach().cpu()
    rows, K = x.shape
    assert q.dtype == torch.uint8 and tuple(q.shape) == (rows, K), what
    assert s.dtype == torch.float32 and tuple(s.shape) == (rows,), what
    s_ref = quant_fp8_scale_ref(x)
    if not torch.equal(s.view(torch.int32), s_ref.view(torch.int32)):
        i = int((s.view(torch.int32) != s_ref.view(torch.int32)).nonzero()[0])
        raise AssertionError(f"{what}: scale of row {i} is {float(s[i])!r}, "
                             f"f32 amax/448 is {float(s_ref[i])!r}")
    t = x.double() / s_ref.double().unsqueeze(1)
    a = t.abs().clamp(max=E4M3_MAX)
    lo, hi = e4m3_neighbours(a)
    mid = (lo + hi) / 2
    g = e4m3_to_f64(q & 0x7f)                      # NaN code 0x7f -> NaN: fails below
    in_pair = (g == lo) | (g == hi)
    nearest = torch.where(a < mid, lo, hi)
    near_mid = fp8_near_midpoint(x, s_ref)
    ok = in_pair & ((g == nearest) | near_mid) & ((q >> 7).bool() == torch.signbit(x))
    if not bool(ok.all()):
        i = tuple(int(v) for v in (~ok).nonzero()[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} elements wrong; first at {i}: "
                             f"x/s = {float(t[i])!r}, got byte 0x{int(q[i]):02x} "
                             f"({float(g[i])!r}), neighbours {float(lo[i])!r} / {float(hi[i])!r}")
    free = ~exact.unsqueeze(1)
    cap = int(FP8_TIE_CAP * x.numel())
    assert int((near_mid & free).sum()) <= cap, f"{what}: generator premise (tie cap)"
    assert int((near_mid & free & (g != nearest)).sum()) <= cap
    if bool(exact.any()):   # scale and quotient exact: one rounding, ties to even
        assert_bytes_equal(q[exact], e4m3_rne_bytes(t[exact]), what + " exact rows")


def check_quant_fp8(fn, rows, K, dev, gen):
    """fn(x [rows, K] bf16) -> (q u8 [rows, K], s f32 [rows]).
    * s == f32 amax / 448 bit for bit (1 for an all-zero row);
    * q is one of the two e4m3 neighbours of x / s (fp64, reference scale),
      with x's sign, and the nearer one unless x / s lies within 4 * 2^-24
      relative of their midpoint (the kernel multiplies by a rounded 1 / s:
      two f32 roundings); at most 0.1% of a call's elements lie that close;
    * rows with amax = 448 * 2^j: bytes equal RNE of the exact quotient."""
    for c, (x, exact) in enumerate(fp8_quant_inputs(gen, rows, K)):
        q, s = fn(x.to(dev))
        judge_quant_fp8(x, exact, q, s, f"quant_fp8 rows={rows} K={K} call {c}")


# --------------------------------------------------------------------------
# MoE combine.  ``fn(down [P,H] bf16, pos [T,k] i32, weight [P] f32) -> [T,H]``
# --------------------------------------------------------------------------
def make_combine_case(gen, T, k, H, mode, pad=5):
    """pos = a true inverse routing permutation: the T*k routed rows sit at
    distinct random slots of a padded layout of P = T*k + pad rows; the pad
    rows carry weight 0 and loud data (64).  mode 'pow2': integer rows in
    [-8, 8], weights 2^-3 .. 2^1 (every partial sum exact); 'random'."""
    P = T * k + pad
    slots = torch.randperm(P, generator=gen)
    pos = slots[:T * k].reshape(T, k).to(torch.int32)
    if mode == "pow2":
        down = torch.randint(-8, 9, (P, H), generator=gen).to(BF16)
        w = torch.exp2(torch.randint(-3, 2, (P,), generator=gen).float())
    else:
        down = rand_bf16(gen, P, H)
        w = (torch.rand(P, generator=gen) + 0.05).float()
    w[slots[T * k:]] = 0.0
    down[slots[T * k:]] = 64.0
    p = pos.long()
    terms = w.double()[p].unsqueeze(-1) * down.double()[p]      # [T, k, H]
    return down, pos, w, terms.sum(dim=1), terms.abs().sum(dim=1)


def check_moe_combine(fn, T, k, H, dev, gen):
    """Bit for bit with power-of-two weights on integer rows; within
    2^-8 |ref| + k 2^-24 sum|w v| on random data."""
    for mode in ("pow2", "random"):
        down, pos, w, ref, absum = make_combine_case(gen, T, k, H, mode)
        got = fn(down.to(dev), pos.to(dev), w.to(dev))
        what = f"moe_combine {mode} T={T} k={k} H={H}"
        if mode == "pow2":
            assert_bits_equal(got, exact_bf16(ref), what)
        else:
            assert tuple(got.shape) == (T, H), what
            assert_within(got, ref, U_BF16_OUT * ref.abs() + k * U_FP32 * absum, what)


# --------------------------------------------------------------------------
# Dense bf16 GEMM.  ``fn(a [M,K] bf16, b [N,K] bf16) -> C = a @ b^T [M,N] bf16``
# --------------------------------------------------------------------------
GEMM_KFACTOR = 1   # check_gemm_random: the bound the grouped bf16 GEMM meets


def gemm_probe_columns(K: int) -> list:
    """Column 0, K - 1 and both sides of every 8 / 16 / 32 / 64 / 128
    boundary: the 16-byte LDS chunk, the pair of chunks one swizzle step
    moves, the k-half of an MFMA step (the ^64-byte read offset), the
    64-element K-tile and the pair of tiles of one double-buffer round."""
    cols = {0, K - 1}
    for step in (8, 16, 32, 64, 128):
        for b in range(step, K, step):
            cols.update((b - 1, b))
    return sorted(c for c in cols if 0 <= c < K)


def gemm_onehot_operand(gen, rows: int, K: int, call: int = 0):
    """[rows, K] bf16 with one non-zero element per row: +-2^e, e in
    [-3, 3], at probe column cols[(call * rows + r) % len(cols)].
    Returns (x, col [rows] int64, val [rows] fp64)."""
    cols = gemm_probe_columns(K)
    col = torch.tensor([cols[(call * rows + r) % len(cols)] for r in range(rows)])
    val = _pow2(torch.randint(-3, 4, (rows,), generator=gen))
    val = val * (torch.randint(0, 2, (rows,), generator=gen).double() * 2 - 1)
    x = torch.zeros(rows, K, dtype=BF16)
    x[torch.arange(rows), col] = val.to(BF16)
    return x, col, val


def gemm_onehot_ncalls(rows: int, K: int) -> int:
    """Calls needed for ``rows`` rows to visit every probe column."""
    return -(-len(gemm_probe_columns(K)) // rows)


def check_gemm_onehot(fn, M, N, K, dev, gen, sides=("a", "b")):
    """One-hot in K on A, then on B (the two operands go through different
    LDS buffers), the other operand random: every C[m, n] is +-2^e times one
    element of the random operand, a bf16 value, and must come out bit for
    bit (the zero products and the fp32 sums of zeros are exact).  Pins the
    chunk swizzle, the k-half offset, the tile <-> LDS slot map and the last
    tile; the random sign and exponent of every row also tell rows apart."""
    for side in sides:
        rows, orows = (M, N) if side == "a" else (N, M)
        other = rand_bf16(gen, orows, K)
        od = other.to(dev)
        for call in range(gemm_onehot_ncalls(rows, K)):
            x, col, val = gemm_onehot_operand(gen, rows, K, call)
            picked = other.double()[:, col]                       # [orows, rows]
            if side == "a":
                ref = picked.t() * val.unsqueeze(1)
                got = fn(x.to(dev), od)
            else:
                ref = picked * val.unsqueeze(0)
                got = fn(od, x.to(dev))
            exp = exact_bf16(ref)
            assert torch.equal(exp.double(), ref), "generator: expectation is not a bf16 value"
            assert_bits_equal(got, exp, f"gemm one-hot in {side.upper()} M={M} N={N} K={K} call {call}")


def gemm_int_operands(gen, M, N, K):
    """A in [-2, 2], B in [-4, 4], every row random."""
    return int_x(gen, M, K), torch.randint(-4, 5, (N, K), generator=gen).to(BF16)


def check_gemm_int(fn, M, N, K, dev, gen):
    """Small integers over all of K: |any partial sum| <= 8 K < 2^24, so the
    fp32 sums are exact in any order and C == bf16_rne(exact sum) bit for
    bit.  The expectation is an fp32 CPU matmul, exact for the same reason.
    Catches a dropped or doubled K-tile, a buffer-parity slip, a swapped or
    duplicated output tile and a wrong C store offset."""
    a, b = gemm_int_operands(gen, M, N, K)
    assert 8 * K < 2 ** 24
    exp = exact_bf16((a.float() @ b.float().t()).double())
    got = fn(a.to(dev), b.to(dev))
    assert_bits_equal(got, exp, f"gemm integer M={M} N={N} K={K}")


def check_gemm_random(fn, M, N, K, dev, gen, kfactor=None):
    """randn operands against the fp64 product, elementwise within
    gemv_bound(ref, |A|.|B|^T, K, GEMM_KFACTOR) = 2^-8 |ref| + K 2^-24
    |A|.|B|^T: bf16 output rounding plus worst-case fp32 summation in any
    order (bf16 x bf16 products are exact in fp32).  Returns (and prints)
    the worst err / bound."""
    a, b = rand_bf16(gen, M, K), rand_bf16(gen, N, K)
    ref = a.double() @ b.double().t()
    absdot = a.double().abs() @ b.double().abs().t()
    bound = gemv_bound(ref, absdot, K, GEMM_KFACTOR if kfactor is None else kfactor)
    got = fn(a.to(dev), b.to(dev))
    what = f"gemm random M={M} N={N} K={K}"
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)}"
    ratio = float(((got.detach().cpu().double() - ref).abs() / bound).max())
    print(f"{what}: max err / bound = {ratio:.3f}")
    assert_within(got, ref, bound, what)
    return ratio


def check_gemm_all(fn, M, N, K, dev, gen):
    check_gemm_onehot(fn, M, N, K, dev, gen)
    check_gemm_int(fn, M, N, K, dev, gen)
    return check_gemm_random(fn, M, N, K, dev, gen)


# --------------------------------------------------------------------------
# Elementwise ops: add_bf16, rmsnorm, fused_add_rmsnorm, swiglu(_padded),
# rope_inplace
# --------------------------------------------------------------------------
def bf16_rne64(v64: torch.Tensor) -> torch.Tensor:
    """Round-to-nearest-even of fp64 values to bf16 in ONE rounding (normal
    range; written out so the expectation never passes through fp32)."""
    a = v64.abs()
    nz = a > 0
    assert float(a[nz].min()) >= 2.0 ** -126 if bool(nz.any()) else True
    _, ex = torch.frexp(a)                       # a = m 2^ex, m in [0.5, 1)
    q = _pow2(ex.long() - 8)                     # bf16 spacing: 8 significand bits
    r = torch.where(nz, torch.round(a / q) * q, torch.zeros_like(a))   # half to even
    return exact_bf16(torch.where(v64 < 0, -r, r))


ADD_PLANTED = [(1.0, 2.0 ** -8, 1.0),                      # tie -> even (down)
               (1.0 + 2.0 ** -7, 2.0 ** -8, 1.0 + 2.0 ** -6),   # tie -> even (up)
               (256.0, 1.0, 256.0), (258.0, 1.0, 260.0),   # ties at another binade
               (-1.0, -(2.0 ** -8), -1.0),
               (1.5, -1.5, 0.0),                           # exact cancellation: +0
               (1.0, 2.0 ** -20, 1.0),                     # far apart: the large one
               (3.0, 2.0 ** -7 + 2.0 ** -8, 3.0 + 2.0 ** -6)]   # just past a tie -> up


def add_inputs(gen, n: int):
    """Two bf16 vectors of n elements: randn times 2^[-6, 6] per element (so
    the exponents of a pair differ), the planted pairs of ADD_PLANTED first."""
    def draw():
        e = torch.randint(-6, 7, (n,), generator=gen)
        return (torch.randn(n, generator=gen, dtype=torch.float64) * _pow2(e)).to(BF16)

    a, b = draw(), draw()
    for i, (x, y, s) in enumerate(ADD_PLANTED[:n]):
        a[i], b[i] = x, y
        assert float(a[i]) == x and float(b[i]) == y, "generator: not bf16 values"
        assert float(bf16_rne64(torch.tensor([x + y], dtype=torch.float64))) == s
    return a, b


def check_add_bf16(fn, n, dev, gen):
    """fn(a, b) -> a + b: bit-equal to RNE of the exact (fp64) sum.  The fp32
    sum the kernel rounds from is exact or, where the exponents are more than
    16 apart, far from any bf16 midpoint, so one rounding is the contract."""
    a, b = add_inputs(gen, n)
    got = fn(a.to(dev), b.to(dev))
    assert_bits_equal(got, bf16_rne64(a.double() + b.double()), f"add_bf16 n={n}")


def rmsnorm_ref64(x, w, eps) -> torch.Tensor:
    xd = x.cpu().double()
    return xd * torch.rsqrt((xd * xd).mean(dim=-1, keepdim=True) + eps) * w.cpu().double()


def rmsnorm_bound(ref64: torch.Tensor, hidden: int) -> torch.Tensor:
    """(2^-8 + (hidden / 2 + 16) 2^-24) |ref|.  2^-8 |ref| is the bf16 output
    rounding.  The fp32 value it rounds from: hidden squares (one rounding
    each) summed in any order are off by at most hidden 2^-24 relative (all
    terms are non-negative), the reciprocal square root halves that; the
    division by hidden, the + eps, rsqrt and the two products are an ulp or
    two each (16 covers them and the (1 + 2^-8) cross term)."""
    return (U_BF16_OUT + (hidden / 2 + 16) * U_FP32) * ref64.abs()


def rmsnorm_pow2_case(gen, rows: int, hidden: int):
    """Rows of +-2^j (j per row), weights +-2^k (k per column), eps = 1e-12:
    the sum of squares hidden 4^j is exact in fp32, the mean is exactly 4^j
    (a correctly rounded division), eps < 2^-39 cannot move it (4^j >= 2^-8),
    so the scale is 2^-j and y = sign(x) w exactly.  Returns (x, w, eps, y)."""
    j = torch.randint(-4, 5, (rows, 1), generator=gen)
    sx = torch.randint(0, 2, (rows, hidden), generator=gen).double() * 2 - 1
    k = torch.randint(-3, 4, (hidden,), generator=gen)
    sw = torch.randint(0, 2, (hidden,), generator=gen).double() * 2 - 1
    x, w = (sx * _pow2(j)).to(BF16), (sw * _pow2(k)).to(BF16)
    eps = 1e-12
    y = exact_bf16(sx * w.double())
    ref = rmsnorm_ref64(x, w, eps)
    assert float(((ref - y.double()).abs() / ref.abs()).max()) < 2.0 ** -30, "generator"
    return x, w, eps, y


def check_rmsnorm(fn, rows, hidden, dev, gen, eps=1e-5):
    """fn(x [rows, hidden], w [hidden], eps) -> y.  Bit-exact on the
    power-of-two case; within rmsnorm_bound of the fp64 reference on randn
    rows of different scales with randn weights."""
    x, w, e0, y = rmsnorm_pow2_case(gen, rows, hidden)
    got = fn(x.to(dev), w.to(dev), e0)
    assert_bits_equal(got, y, f"rmsnorm power-of-two rows={rows} hidden={hidden}")
    scale = _pow2(torch.randint(-3, 4, (rows, 1), generator=gen))
    x = (torch.randn(rows, hidden, generator=gen, dtype=torch.float64) * scale).to(BF16)
    w = rand_bf16(gen, hidden)
    ref = rmsnorm_ref64(x, w, eps)
    got = fn(x.to(dev), w.to(dev), eps)
    assert_within(got, ref, rmsnorm_bound(ref, hidden),
                  f"rmsnorm random rows={rows} hidden={hidden}")


def check_fused_add_rmsnorm(fn, rows, hidden, dev, gen, eps=1e-5):
    """fn(x, res, w, eps) -> (y, res_out).  res_out is bit-equal to RNE(x +
    res); y is the norm of that ROUNDED sum (what the kernel re-reads), bit
    for bit on the power-of-two case (x = res = +-2^(j-1)) and within
    rmsnorm_bound on the add_inputs data."""
    x, w, e0, y = rmsnorm_pow2_case(gen, rows, hidden)
    half = (x.double() / 2).to(BF16)
    got, r = fn(half.to(dev), half.clone().to(dev), w.to(dev), e0)
    what = f"fused_add_rmsnorm rows={rows} hidden={hidden}"
    assert_bits_equal(r, x, what + " power-of-two residual")
    assert_bits_equal(got, y, what + " power-of-two y")
    a, b = add_inputs(gen, rows * hidden)
    a, b = a.view(rows, hidden), b.view(rows, hidden)
    w = rand_bf16(gen, hidden)
    got, r = fn(a.to(dev), b.clone().to(dev), w.to(dev), eps)
    r_exp = bf16_rne64(a.double() + b.double())
    assert_bits_equal(r, r_exp, what + " residual")
    ref = rmsnorm_ref64(r_exp, w, eps)
    assert_within(got, ref, rmsnorm_bound(ref, hidden), what + " y")


SWIGLU_EDGE_G = [0.0, 32.0, -32.0, 8.0, -8.0, 0.5, -0.5, 2.0 ** -20]


def swiglu_inputs(gen, rows: int, inter: int) -> torch.Tensor:
    """gateup [rows, 2 inter]: 2 randn, with SWIGLU_EDGE_G planted in the
    first and in the last 8-vector of row 0's gate (up = 1.5 there)."""
    gu = (torch.randn(rows, 2 * inter, generator=gen) * 2).to(BF16)
    if rows:
        edge = torch.tensor(SWIGLU_EDGE_G, dtype=BF16)
        for c0 in (0, inter - 8):
            gu[0, c0:c0 + 8] = edge
            gu[0, inter + c0:inter + c0 + 8] = 1.5
    return gu


def swiglu_bound(gateup: torch.Tensor) -> torch.Tensor:
    """(2^-8 + (2 |g| + 8) 2^-24) |ref| around swiglu_ref64.  The kernel
    takes exp(-g) as exp2(-g log2 e) in fp32: the rounded constant and the
    rounded product each move the exponent by |g log2 e| 2^-24, the result by
    |g| 2^-24 relative, and 1 + exp(-g) no more than that; v_exp_f32, the
    sum, the division and the product with u are an ulp or two each."""
    g = gateup.cpu().double()[..., :gateup.shape[-1] // 2]
    return (U_BF16_OUT + (2 * g.abs() + 8) * U_FP32) * swiglu_ref64(gateup).abs()


def check_swiglu(fn, fn_padded, rows, inter, dev, gen):
    """fn(gateup) -> [rows, inter] within swiglu_bound; fn_padded(gateup,
    out_rows) for out_rows = rows, rows + 1 and rows + 3: the first rows
    bit-equal to fn's, the pad rows +0.  silu(32) = 32 and silu(0) = 0 come
    out exactly (1 + exp(-32) == 1 in fp32)."""
    gu = swiglu_inputs(gen, rows, inter)
    gd = gu.to(dev)
    what = f"swiglu rows={rows} inter={inter}"
    y = None
    if rows:
        y = fn(gd)
        assert tuple(y.shape) == (rows, inter), what
        assert_within(y, swiglu_ref64(gu), swiglu_bound(gu), what)
        yc = y.detach().cpu().float()
        for c0 in (0, inter - 8):
            assert float(yc[0, c0]) == 0.0 and float(yc[0, c0 + 1]) == 48.0, what + " edges"
    for out_rows in (rows, rows + 1, rows + 3):
        yp = fn_padded(gd, out_rows)
        assert tuple(yp.shape) == (out_rows, inter), f"{what} out_rows={out_rows}"
        if rows:
            assert_bits_equal(yp[:rows].contiguous(), y, f"{what} out_rows={out_rows} head")
        pad = bits(yp[rows:].contiguous())
        assert bool((pad == 0).all()), f"{what} out_rows={out_rows}: pad rows are not +0"


def check_rope_inplace(fn, Hq, Hk, D, dev, gen, rope_tables, max_pos=300):
    """fn(q [T,Hq,D], k [T,Hk,D], cos_sin, positions) rotates in place.
    Positions repeat and include 0 (cos = 1, sin = 0: bit-equal to the input)
    and max_pos - 1; every element within the rope_ref64 bound."""
    pos = torch.tensor([0, 5, 5, max_pos - 1, 0, 17, 5], dtype=torch.int32)
    T = pos.numel()
    q0, k0 = rand_bf16(gen, T, Hq, D), rand_bf16(gen, T, Hk, D)
    cs = rope_tables(max_pos, D, 500000.0)
    q, k = q0.clone().to(dev), k0.clone().to(dev)
    fn(q, k, cs.to(dev), pos.to(dev))
    what = f"rope_inplace Hq={Hq} Hk={Hk} D={D}"
    for got, x0, nm in ((q, q0, "q"), (k, k0, "k")):
        r64, bnd = rope_ref64(x0, cs, pos)
        assert_within(got, r64, bnd, f"{what} {nm}")
        z = (pos == 0).nonzero().flatten()
        assert_bits_equal(got.cpu()[z].contiguous(), x0[z].contiguous(),
                          f"{what} {nm} at position 0")
        same = (pos == 5).nonzero().flatten()      # the table row is shared, not the data
        assert not torch.equal(got.cpu()[same[0]], got.cpu()[same[1]])
