"""Edge-shape exactness tests for the decode path on the GPU: the GEMV family,
paged decode attention, rope_kv_append / rope_scatter_qkv and the sampling
epilogues, each against the fp64 oracles in tests/kernel_oracles.py.

Three kinds of check (see kernel_oracles for the derivations):
  * one-hot probes and small-integer data -> bit-exact;
  * random data -> elementwise bound from bf16 output rounding (2^-8 |ref|)
    plus the worst-case fp32 summation error (K 2^-24 |x|.|w|^T);
  * fused swiglu (activation rounded to bf16 in LDS) -> relative Frobenius
    error <= 2^-8.
Shapes are the smallest that reach each path: every M bucket, the smallest
legal K, N tails, slot / step / ring-wrap boundaries, dispatch thresholds.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_oracles as ko
from senweaver_amd import ops

M_BF16 = [1, 2, 3, 4, 5, 8, 9, 16]
M_FP8 = [1, 2, 3, 4, 5, 8]
N_ANY = [4, 12, 260]
N_8 = [8, 24, 264]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_loaded(), "HIP extension failed to build/load"
    return torch.device("cuda:0")


@pytest.fixture
def gen():
    return torch.Generator().manual_seed(20240)


def _v3(x, w):
    return ops.hip_ext().gemv_bt_v3(x, w)


def _swiglu_ext(gu, w):
    return ops.hip_ext().swiglu_gemv_bt(gu, w)


# ---------------- GEMV family ----------------
@pytest.mark.parametrize("K", [512, 1536, 4096])
def test_gemv_v2_bit_exact(dev, gen, K):
    """bf16 v2 GEMV through ops.gemm_bt, every M bucket (1, 2, 4, 8, 16) and
    the padded M in between, N tails 4 / 12 / 260."""
    ko.check_gemv_onehot(ops.gemm_bt, "bf16", M_BF16, N_ANY, K, dev, gen)
    ko.check_gemv_int(ops.gemm_bt, "bf16", M_BF16, N_ANY, K, dev, gen)


@pytest.mark.parametrize("K", [512, 1536, 4096])
def test_gemv_v2_random(dev, gen, K):
    ko.check_gemv_random(ops.gemm_bt, "bf16", M_BF16, N_ANY, K, dev, gen)


@pytest.mark.parametrize("K", [1024, 4096, 5120, 14336])
def test_gemv_v3_bit_exact(dev, gen, K):
    """Streaming GEMV: the K <= 4096 kernel (1024: one step, no ring refill;
    4096: ring wrap at slot 6) and the wide kernel (5120: smallest; 14336:
    full x capacity), through the raw binding."""
    ko.check_gemv_onehot(_v3, "bf16", [1], N_8, K, dev, gen)
    ko.check_gemv_int(_v3, "bf16", [1], N_8, K, dev, gen)


@pytest.mark.parametrize("K", [1024, 4096, 5120, 14336])
def test_gemv_v3_random(dev, gen, K):
    ko.check_gemv_random(_v3, "bf16", [1], N_8, K, dev, gen)


@pytest.mark.parametrize("K", [512, 1536])
def test_gemv_v3_rejects_odd_slot_count(dev, K):
    """Both streaming kernels walk K in 1024-element steps: K % 1024 != 0
    would drop the last 512 columns (and K = 512 would read past each row),
    so the binding must refuse.  Host-side check; nothing is launched."""
    x = torch.zeros(1, K, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(8, K, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError):
        _v3(x, w)


def test_gemv_bindings_reject_mismatched_operands(dev):
    """The kernels index every operand from M, N, K alone, so the bindings
    must refuse operands of another size.  Host-side checks; each mismatch
    is an operand that is too LARGE, so nothing here could read out of
    bounds even if a check were missing."""
    ext = ops.hip_ext()
    bf = dict(dtype=torch.bfloat16, device=dev)
    M, N, K = 2, 8, 1024
    x, w = torch.zeros(M, K, **bf), torch.zeros(N, K, **bf)
    with pytest.raises(RuntimeError):   # weight rows longer than x
        ext.gemv_bt_v3(x[:1], torch.zeros(N, 2 * K, **bf))
    with pytest.raises(RuntimeError):   # norm weight of another length
        ext.gemv_norm_bt(x, None, torch.zeros(2 * K, **bf), w, 1e-5)
    with pytest.raises(RuntimeError):   # residual with another row count
        ext.gemv_norm_bt(x, torch.zeros(M + 1, K, **bf), torch.zeros(K, **bf), w, 1e-5)
    q = torch.zeros(N, K, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError):   # one scale per row, no more
        ext.gemv_bt_fp8w(x, q, torch.ones(N + 4, dtype=torch.float32, device=dev))
    with pytest.raises(RuntimeError):   # [N, K/32] block scales
        ext.gemv_bt_mxfp8w(x, q, torch.zeros(N + 4, K // 32, dtype=torch.uint8, device=dev))


@pytest.mark.parametrize("kind", ["fp8", "mx"])
@pytest.mark.parametrize("K", [1024, 3072, 4096])
def test_gemv_fp8_weights_bit_exact(dev, gen, kind, K):
    """fp8w (1 row/wave at M=1, 2 rows/wave above: N=12 leaves a half-used
    wave) and mxfp8w, weights built directly from bytes with power-of-two
    scales."""
    fn = ops.gemv_fp8w if kind == "fp8" else ops.gemv_mxfp8w
    ko.check_gemv_onehot(fn, kind, M_FP8, N_ANY, K, dev, gen)
    ko.check_gemv_int(fn, kind, M_FP8, N_ANY, K, dev, gen)


@pytest.mark.parametrize("kind", ["fp8", "mx"])
@pytest.mark.parametrize("K", [1024, 3072, 4096])
def test_gemv_fp8_weights_random(dev, gen, kind, K):
    fn = ops.gemv_fp8w if kind == "fp8" else ops.gemv_mxfp8w
    ko.check_gemv_random(fn, kind, M_FP8, N_ANY, K, dev, gen,
                         mode="random_scale" if kind == "fp8" else "random")


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("K", [512, 1536, 4096])
def test_gemv_norm(dev, gen, K, with_res):
    """Fused add + RMSNorm + GEMV: random data and one-hot probes within the
    2K bound (rsqrt keeps it from being bit-exact); res_out bit-equal."""
    ko.check_gemv_norm(ops.gemv_norm_bt, M_BF16, N_ANY, K, dev, gen, with_res)
    ko.check_gemv_norm(ops.gemv_norm_bt, M_BF16, [12], K, dev, gen, with_res, onehot=True)


@pytest.mark.parametrize("K", [5120, 14336])
def test_swiglu_gemv_fused(dev, gen, K):
    ko.check_swiglu_onehot(_swiglu_ext, N_8, K, dev, gen)
    ko.check_swiglu_random(_swiglu_ext, N_8, K, dev, gen)


@pytest.mark.parametrize("N", [12, 264])
@pytest.mark.parametrize("K", [4096, 5120, 14336, 15360])
def test_gemm_bt_dispatch_boundaries(dev, gen, K, N):
    """M=1 through ops.gemm_bt on both sides of the v2 / streaming-kernel
    thresholds (K 4096|5120, 14336|15360, N % 8): same checks whichever
    kernel serves the shape."""
    ko.check_gemv_onehot(ops.gemm_bt, "bf16", [1], [N], K, dev, gen)
    ko.check_gemv_int(ops.gemm_bt, "bf16", [1], [N], K, dev, gen)
    ko.check_gemv_random(ops.gemm_bt, "bf16", [1], [N], K, dev, gen)


@pytest.mark.parametrize("N", [12, 264])
@pytest.mark.parametrize("K", [4096, 5120])
def test_swiglu_gemv_dispatch_boundaries(dev, gen, K, N):
    ko.check_swiglu_onehot(ops.swiglu_gemv, [N], K, dev, gen)
    ko.check_swiglu_random(ops.swiglu_gemv, [N], K, dev, gen)


# ---------------- paged decode attention ----------------
@pytest.mark.parametrize("ctx", [1, 7, 9, 16, 17, 33, 257, 1032, 2100])
def test_paged_attn_onehot(dev, gen, ctx):
    """K[p*] = 16 q: the probed head must return V[p*] bit for bit.  Reaches
    the empty splits (ctx < 8), a wave's second / third pass (ctx > 1024),
    all four waves live and the last split's short tail."""
    ko.check_paged_onehot(ops.paged_decode_attn, ctx, dev, gen)


@pytest.mark.parametrize("mode", ["diffuse", "peaked", "late_spike"])
@pytest.mark.parametrize("H,Hk", [(2, 2), (8, 2), (16, 2)])
def test_paged_attn_random(dev, gen, H, Hk, mode):
    ko.check_paged_random(ops.paged_decode_attn, (1, 1032, 2100), H, Hk, dev, gen, mode)


# ---------------- rope ----------------
@pytest.mark.parametrize("Hq,Hk,D", [(32, 8, 128), (4, 2, 64)])
def test_rope_kv_append_edges(dev, gen, Hq, Hk, D):
    """(32, 8, 128): 48 heads = two y-blocks, the second partial.  Sentinel-
    filled caches: every row not named in ``slot`` must be untouched."""
    ko.check_rope_kv_append(ops.rope_kv_append, Hq, Hk, D, dev, gen, ops.rope_tables)


@pytest.mark.parametrize("Hq,Hk,D", [(32, 8, 128), (4, 2, 64)])
def test_rope_scatter_edges(dev, gen, Hq, Hk, D):
    ko.check_rope_scatter(ops.rope_scatter_qkv, Hq, Hk, D, dev, gen, ops.rope_tables,
                          B=2, S=64)


# ---------------- sampling ----------------
@pytest.mark.parametrize("vocab", [8, 512, 1000, 2048, 2056, 128256])
def test_argmax_rows_edges(dev, gen, vocab):
    ko.check_argmax(ops.argmax_rows, vocab, dev, gen)


def test_argmax_rows_scalar_tail(dev, gen):
    """vocab = 1003 exercises the scalar tail loop.  ONE row per call: with
    vocab % 8 != 0 every later row would start off 16-byte alignment for the
    kernel's vector loads; that multi-row case is deliberately not tested."""
    ko.check_argmax(ops.argmax_rows, 1003, dev, gen, single_rows=True)


@pytest.mark.parametrize("vocab", [8, 512, 1000, 2048, 128256])
def test_target_logprob_edges(dev, gen, vocab):
    """Small vocab leaves threads (and whole waves) without an element;
    -inf logits include a thread's first element.  All outputs finite."""
    ko.check_target_logprob(ops.target_logprob, vocab, dev, gen)
