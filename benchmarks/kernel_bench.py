"""Micro-benchmarks for the gfx950 kernels (run on an MI355X via gpurun).

Prints TFLOP/s for GEMM/attention and GB/s for the memory-bound ops.
Random data (never zero-filled — DVFS inflates zero-fill numbers).
"""

import math
import sys
import time

import torch

sys.path.insert(0, ".")
from senweaver_amd import ops  # noqa: E402


def timeit(fn, warmup=5, iters=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_gemm():
    dev = torch.device("cuda:0")
    shapes = [
        (4096, 4096, 4096),
        (8192, 8192, 8192),
        (2048, 6144, 4096),    # llama-8B qkv
        (2048, 28672, 4096),   # llama-8B gate|up
        (2048, 4096, 14336),   # llama-8B down
        (2048, 128256, 4096),  # lm_head
    ]
    for M, N, K in shapes:
        a = torch.randn(M, K, dtype=torch.bfloat16, device=dev)
        b = torch.randn(N, K, dtype=torch.bfloat16, device=dev)
        t = timeit(lambda: ops.gemm_bt_tiled(a, b))
        tf = 2 * M * N * K / t / 1e12
        # hipBLASLt comparison point
        bt = b.t().contiguous().t()  # keep layout; torch matmul uses blas
        t2 = timeit(lambda: a @ b.t())
        tf2 = 2 * M * N * K / t2 / 1e12
        print(f"GEMM {M}x{N}x{K}: ours {tf:7.1f} TF/s   hipblaslt {tf2:7.1f} TF/s")


def event_us(fn, n_rot, warmup=3, iters=10):
    """Device time per call in us; fn(i) runs on rotation slot i % n_rot."""
    for i in range(warmup):
        fn(i % n_rot)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(iters):
        fn((warmup + i) % n_rot)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def gemm_lt_table(M, N, K, transposed=False, verbose=True, label=""):
    """The tuner's candidate table for one GEMM, next to torch.matmul on the
    same inputs.  B rotates over enough distinct buffers to exceed the
    256 MB Infinity Cache, so every timing reads its weights from HBM."""
    dev = torch.device("cuda:0")
    ext = ops.hip_ext()
    n_rot = max(1, min(32, -(-(320 << 20) // (N * K * 2))))
    bs = [torch.randn(N, K, dtype=torch.bfloat16, device=dev) for _ in range(n_rot)]
    if transposed:
        a = torch.randn(K, M, dtype=torch.bfloat16, device=dev).t()
    else:
        a = torch.randn(M, K, dtype=torch.bfloat16, device=dev)
    t_torch = [event_us(lambda i: torch.matmul(a, bs[i].t()), n_rot) for _ in range(3)]
    r = ext.gemm_lt_tune(a, bs[0], 0, bs, True)
    t_lt = [event_us(lambda i: ext.gemm_lt(a, bs[i]), n_rot) for _ in range(3)]
    cands = r["candidates"]
    timed = [c for c in cands if c["status"] == "timed"]
    fl = 2.0 * M * N * K
    lay = "A^T view" if transposed else "row-major"
    print(f"{label or 'gemm'} M={M} N={N} K={K} {lay}: status {r['status']}, "
          f"{len(cands)} candidates ({len(timed)} timed in full, "
          f"{sum(c['status'] == 'not reproducible' for c in cands)} not reproducible), "
          f"tuning took {r['tune_ms']:.0f} ms, rotation {n_rot} x {N * K * 2 >> 20} MB")
    print(f"  torch.matmul        {min(t_torch):8.1f} us  (3 runs: "
          f"{' '.join(f'{t:.1f}' for t in t_torch)})  {fl / min(t_torch) / 1e9:.3f} PF/s")
    print(f"  first choice        {r['first_us']:8.1f} us  [{cands[0]['index']}] {cands[0]['name'][:90]}")
    ch = cands[r["chosen"]]
    print(f"  chosen (cand {r['chosen']:3d})   {r['best_us']:8.1f} us  [{ch['index']}] {ch['name'][:90]}"
          f"  {fl / r['best_us'] / 1e9:.3f} PF/s")
    print(f"  gemm_lt as routed   {min(t_lt):8.1f} us  (3 runs: {' '.join(f'{t:.1f}' for t in t_lt)})")
    if verbose:
        for c in cands:
            us = f"{c['us']:8.1f}" if "us" in c else "        "
            fr = f"{c['first_run_us']:8.1f}" if "first_run_us" in c else "        "
            print(f"    cand {c['cand']:3d} idx {c['index']:6d} first {fr} avg {us} us  {c['status']}")
    return min(t_torch), r["first_us"], r["best_us"]


def bench_gemm_lt(argv):
    """kernel_bench.py gemm_lt M N K [t]   one GEMM's candidate table
    kernel_bench.py gemm_lt bench       the headline bench's GEMM shapes"""
    if argv and argv[0] != "bench":
        M, N, K = (int(v) for v in argv[:3])
        gemm_lt_table(M, N, K, transposed=len(argv) > 3 and argv[3] == "t")
        return
    Tp, BS = 6848, 8192   # llama-3-8b, mb4, seq 2048, 500 shared tokens, G=64
    rows = []
    for label, M, N, K, t in (("qkv", Tp, 6144, 4096, False),
                              ("gate|up", Tp, 28672, 4096, False),
                              ("o_proj", Tp, 4096, 4096, True),
                              ("o_proj", Tp, 4096, 4096, False),
                              ("down", Tp, 4096, 14336, False),
                              ("down", BS, 4096, 14336, False),
                              ("lm_head", 1600, 128256, 4096, False)):
        rows.append((label, M, t) + gemm_lt_table(M, N, K, t, verbose=False, label=label))
        torch.cuda.empty_cache()
    print("summary (us): GEMM, M, layout, torch.matmul, first choice, best")
    for label, M, t, tt, tf, tb in rows:
        print(f"  {label:8s} {M:5d} {'A^T' if t else 'row'}  {tt:8.1f} {tf:8.1f} {tb:8.1f}")


def bench_gemm8():
    """The pipelined 256-tile kernels (v14, asm4 = 21, asm7 = 24) vs hipBLASLt."""
    dev = torch.device("cuda:0")
    ext = ops.hip_ext()
    shapes = [
        (4096, 4096, 4096),
        (8192, 8192, 8192),
        (2048, 6144, 4096),
        (2048, 28672, 4096),
        (2048, 4096, 14336),
        (2048, 128256, 4096),
    ]
    for M, N, K in shapes:
        a = torch.randn(M, K, dtype=torch.bfloat16, device=dev)
        b = torch.randn(N, K, dtype=torch.bfloat16, device=dev)
        fl = 2 * M * N * K / 1e12
        ts = {var: timeit(lambda: ext.gemm_bt_8ph_v(a, b, var)) for var in (14, 21, 24)}
        tb = timeit(lambda: a @ b.t())
        print(f"GEMM8 {M}x{N}x{K}: " +
              "  ".join(f"v{var} {fl / t:7.1f}" for var, t in ts.items()) +
              f" TF/s   hipblaslt {fl / tb:7.1f} TF/s")
        # numerics spot-check on the fly (fp32 reference is expensive at 8k;
        # compare vs blas bf16 result within bf16 tolerance)
        cb = (a @ b.t()).float()
        den = cb.abs().max().item()
        for var in ts:
            err = (ext.gemm_bt_8ph_v(a, b, var).float() - cb).abs().max().item()
            print(f"      v{var} max|d| {err:.3f} (ref max {den:.1f})")


def bench_fp8():
    dev = torch.device("cuda:0")
    shapes = [(4096, 4096, 4096), (8192, 8192, 8192), (2048, 28672, 4096)]
    for M, N, K in shapes:
        a = torch.randn(M, K, dtype=torch.bfloat16, device=dev)
        b = torch.randn(N, K, dtype=torch.bfloat16, device=dev)
        aq, asc = ops.quant_fp8(a)
        bq, bsc = ops.quant_fp8(b)
        t = timeit(lambda: ops.gemm_bt_fp8(aq, asc, bq, bsc))
        amq, ams = ops.quant_mxfp8(a)
        bmq, bms = ops.quant_mxfp8(b)
        tm = timeit(lambda: ops.gemm_bt_mxfp8(amq, ams, bmq, bms))
        tq = timeit(lambda: ops.quant_mxfp8(a))
        fl = 2 * M * N * K / 1e12
        print(f"FP8  {M}x{N}x{K}: rowwise {fl / t:7.1f} TF/s   mx-scaled {fl / tm:7.1f}"
              f" TF/s   (quant_mx {M * K * 2 / tq / 1e9:5.0f} GB/s)")


def bench_tile():
    """The six single-barrier tile GEMMs of gemm.hip / moe.hip / fp8.hip, each
    at a shape whose dispatch reaches it (the asm / v14 kernels and the vendor
    library take the other shapes).  Device time by events, 5 repeats each."""
    dev = torch.device("cuda:0")
    ext = ops.hip_ext()

    def bf16(*shape):
        return torch.randn(*shape, dtype=torch.bfloat16, device=dev)

    def dense(M, N, K):
        a, b = bf16(M, K), bf16(N, K)
        return lambda: ext.gemm_bt(a, b)

    def grouped(E, rows, N, K):
        # the tile map ops.grouped_gemm_bt builds under SENWEAVER_GEMM=hip
        a, w = bf16(E * rows, K), bf16(E, N, K)
        m0 = list(range(0, E * rows, 128))
        te = torch.tensor([m // rows for m in m0], dtype=torch.int32, device=dev)
        tm = torch.tensor(m0, dtype=torch.int32, device=dev)
        ends = torch.tensor([(e + 1) * rows for e in range(E)], dtype=torch.int32, device=dev)
        return lambda: ext.grouped_gemm_bt(a, w, te, tm, ends)

    def quant(M, N, K, q, gemm):
        (aq, asc), (bq, bsc) = q(bf16(M, K)), q(bf16(N, K))
        return lambda: gemm(aq, asc, bq, bsc)

    cases = [
        ("gemm_bt_bf16_kernel", (2048, 4096, 4096), dense),          # 128 256-tiles < 160
        ("gemm_bt_bf16_256_kernel", (4096, 4096, 4160), dense),      # K % 128 == 64
        ("grouped_gemm_bt_bf16_kernel", (8 * 1024, 14336, 4096),
         lambda M, N, K: grouped(8, 1024, N, K)),
        ("gemm_bt_fp8_kernel", (4096, 4096, 4096),
         lambda M, N, K: quant(M, N, K, ext.quant_fp8, ext.gemm_bt_fp8)),
        ("gemm_bt_mxfp8_kernel", (2048, 4096, 4096),
         lambda M, N, K: quant(M, N, K, ext.quant_mxfp8, ext.gemm_bt_mxfp8)),
        ("gemm_bt_mxfp8_256_kernel", (8192, 8192, 8192),
         lambda M, N, K: quant(M, N, K, ext.quant_mxfp8, ext.gemm_bt_mxfp8)),
    ]
    for name, (M, N, K), make in cases:
        fn = make(M, N, K)
        us = sorted(event_us(lambda i: fn(), 1, warmup=5, iters=20) for _ in range(5))
        fl = 2.0 * M * N * K
        print(f"TILE {name:28s} {M}x{N}x{K}: median {us[2]:8.1f} us  "
              f"{fl / us[2] / 1e6:7.1f} TF/s  (runs: {' '.join(f'{u:.1f}' for u in us)})")
        del fn
        torch.cuda.empty_cache()


def bench_attn():
    dev = torch.device("cuda:0")
    for (B, H, Hk, S) in [(4, 32, 8, 2048), (2, 32, 8, 4096), (1, 32, 8, 8192)]:
        D = 128
        q = torch.randn(B, H, S, D, dtype=torch.bfloat16, device=dev)
        k = torch.randn(B, Hk, S, D, dtype=torch.bfloat16, device=dev)
        v = torch.randn(B, Hk, S, D, dtype=torch.bfloat16, device=dev)
        vt = v.transpose(-1, -2).contiguous()
        scale = 1.0 / math.sqrt(D)
        ext = ops.hip_ext()
        t2 = timeit(lambda: ext.attn_fwd_v2(q, k, vt, scale))
        t3 = timeit(lambda: ext.attn_fwd_v3(q, k, vt, scale))
        t5 = timeit(lambda: ext.attn_fwd_v5(q, k, vt, scale))
        flops = 2 * 2 * B * H * S * S * D / 2  # causal half
        print(f"ATTN B{B} H{H} S{S}: v2 {flops / t2 / 1e12:7.1f}  v3 {flops / t3 / 1e12:7.1f}  v5 {flops / t5 / 1e12:7.1f} TF/s")
        tsdpa = timeit(lambda: torch.nn.functional.scaled_dot_product_attention(
            q, k, v, is_causal=True, enable_gqa=True))
        print(f"  torch sdpa:        {flops / tsdpa / 1e12:7.1f} TF/s")


def bench_attn_packed(rounds=5):
    """The packed prefill attention of the headline shape (B4 H32 Hk8 S2048,
    skips 0/448/448/448), V^T route against V-rows route, alternating in one
    session: attn_fwd_v5_packed_rm on a ready V^T, vt_from_qkv_packed (the
    pass the new kernel makes unnecessary), and attn_fwd_v5_packed_rm_qkv.
    Device time per call in us, three rotating input sets."""
    from senweaver_amd.engine.prefix_plan import plan_from_skips
    dev = torch.device("cuda:0")
    ext = ops.hip_ext()
    B, H, Hk, S, D = 4, 32, 8, 2048, 128
    plan = plan_from_skips((0,) * B, (0, 448, 448, 448), S)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    skip, base, owner = i32(plan.skip), i32(plan.base), i32(plan.owner)
    scale = 1.0 / math.sqrt(D)
    sets = []
    for _ in range(3):
        q = torch.randn(B, H, S, D, dtype=torch.bfloat16, device=dev)
        k = torch.randn(B, Hk, S, D, dtype=torch.bfloat16, device=dev)
        qkv = torch.randn(plan.Tp, (H + 2 * Hk) * D, dtype=torch.bfloat16, device=dev)
        vt = ext.vt_from_qkv_packed(qkv, H, Hk, D, B, S, skip, base, owner)
        sets.append((q, k, qkv, vt, torch.empty(plan.Tp, H * D, dtype=torch.bfloat16, device=dev)))
    old = lambda i: ext.attn_fwd_v5_packed_rm(sets[i][0], sets[i][1], sets[i][3], scale,
                                              skip, base, plan.Tp, sets[i][4])
    tr = lambda i: ext.vt_from_qkv_packed(sets[i][2], H, Hk, D, B, S, skip, base, owner)
    new = lambda i: ext.attn_fwd_v5_packed_rm_qkv(sets[i][0], sets[i][1], sets[i][2], H, Hk,
                                                  scale, skip, base, owner, plan.Tp, sets[i][4])
    print(f"ATTN packed B{B} H{H} Hk{Hk} S{S} skips {plan.skip} Tp {plan.Tp}: us per call")
    print("  round   V^T attn   V^T pass   sum     V-rows attn")
    for r in range(rounds):
        t_old, t_tr, t_new = (event_us(f, 3, warmup=3, iters=30) for f in (old, tr, new))
        print(f"  {r:5d}   {t_old:8.1f}   {t_tr:8.1f}   {t_old + t_tr:6.1f}   {t_new:8.1f}")


def bench_gemv():
    """Decode GEMV family: bf16 v2/v3(engine) and fp8/mxfp8-weight forms."""
    dev = torch.device("cuda:0")
    ext = ops.hip_ext()
    for (name, N, K) in [("qkv", 6144, 4096), ("gateup", 28672, 4096),
                         ("down", 4096, 14336)]:
        x = torch.randn(1, K, dtype=torch.bfloat16, device=dev)
        w = torch.randn(N, K, dtype=torch.bfloat16, device=dev)
        wq, ws = ops.quant_fp8(w)
        mq, ms = ops.quant_mxfp8(w)
        t2 = timeit(lambda: ext.gemm_bt(x, w))
        t3 = timeit(lambda: ext.gemv_bt_v3(x, w))
        tf = timeit(lambda: ext.gemv_bt_fp8w(x, wq, ws))
        tm = timeit(lambda: ext.gemv_bt_mxfp8w(x, mq, ms))
        gb = N * K * 2
        print(f"GEMV {name:7s} N{N} K{K}: v2 {gb/t2/1e12:5.2f}  v3 {gb/t3/1e12:5.2f}"
              f"  fp8w {gb/2/tf/1e12:5.2f}  mxfp8w {gb/2/tm/1e12:5.2f} TB/s"
              f"  (fp8w speedup vs v2 {t2/tf:4.2f}x)")


def bench_memops():
    dev = torch.device("cuda:0")
    x = torch.randn(8192, 4096, dtype=torch.bfloat16, device=dev)
    w = torch.randn(4096, dtype=torch.bfloat16, device=dev)
    t = timeit(lambda: ops.rmsnorm(x, w, 1e-5))
    gb = 2 * x.numel() * 2 / t / 1e9
    print(f"RMSNorm 8192x4096: {gb:7.0f} GB/s")
    res = torch.randn_like(x)
    t = timeit(lambda: ops.fused_add_rmsnorm(x, res, w, 1e-5))
    gb = 4 * x.numel() * 2 / t / 1e9
    print(f"FusedAddRMSNorm:   {gb:7.0f} GB/s")
    gu = torch.randn(8192, 2 * 14336, dtype=torch.bfloat16, device=dev)
    t = timeit(lambda: ops.swiglu(gu))
    gb = (gu.numel() + gu.numel() // 2) * 2 / t / 1e9
    print(f"SwiGLU 8192x14336: {gb:7.0f} GB/s")
    logits = torch.randn(2048, 128256, dtype=torch.bfloat16, device=dev)
    tgt = torch.randint(0, 128256, (2048,), dtype=torch.int32, device=dev)
    t = timeit(lambda: ops.target_logprob(logits, tgt))
    gb = logits.numel() * 2 / t / 1e9
    print(f"TargetLogprob:     {gb:7.0f} GB/s")


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which in ("all", "gemm"):
        bench_gemm()
    if which == "gemm_lt":
        bench_gemm_lt(sys.argv[2:])
    if which == "gemm8":
        bench_gemm8()
    if which in ("all", "fp8"):
        bench_fp8()
    if which == "tile":
        bench_tile()
    if which in ("all", "attn"):
        bench_attn()
    if which == "attn_packed":
        bench_attn_packed()
    if which in ("all", "gemv"):
        bench_gemv()
    if which in ("all", "mem"):
        bench_memops()
