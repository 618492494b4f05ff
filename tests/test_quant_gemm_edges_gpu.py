"""Exactness tests for the quantized prefill path and the MoE path on the
GPU: the tiled fp8 / mxfp8 GEMM kernels, the grouped bf16 GEMM, the two
quantizers and moe_combine, each against the fp64 oracles in
tests/kernel_oracles.py.

The in-repo kernels are reached directly: through the raw bindings, and
through ops.* with ``_GEMM_IMPL = "hip"`` (the default "auto" hands fp8 and
grouped GEMMs to the vendor library, which would leave gemm_bt_fp8_kernel and
grouped_gemm_bt_bf16_kernel unrun).

Kinds of check (derivations in kernel_oracles):
  * one-hot in K with power-of-two scales, a different exponent for every
    (row, 32-block) on mx -> bit-exact; pins the scale byte <-> K block map;
  * small integers over all of K -> bit-exact;
  * random bytes and scales -> bf16 rounding + worst-case fp32 summation;
  * quantizers -> scale bytes / f32 scales equal, payload bytes equal (mx,
    exact fp8 rows) or the nearest e4m3 neighbour (fp8).
Shapes are the smallest that reach each path: 1 / 6 / 9 / 20 workgroups (the
XCD remap's small-count and remainder branches), K of one to five tiles, the
M-padding fallbacks, both sides of the 160-tile threshold of the 256 kernel.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_oracles as ko
from senweaver_amd import ops

MN = [(128, 128), (256, 384), (384, 384), (512, 640)]     # 1, 6, 9, 20 workgroups
KS = [128, 256, 384, 640]                                 # 128: no prefetch
M_PAD = [1, 17, 130, 200]
SIZES = [[0, 1, 127, 128, 129, 0, 300, 5], [0, 0, 0, 0, 0, 0, 0, 77], [130, 0, 0, 0],
         [128, 128]]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_loaded(), "HIP extension failed to build/load"
    return torch.device("cuda:0")


@pytest.fixture
def gen():
    return torch.Generator().manual_seed(77031)


@pytest.fixture
def hip_impl(monkeypatch):
    """ops.* routes to the in-repo kernels, as SENWEAVER_GEMM=hip does."""
    monkeypatch.setattr(ops, "_GEMM_IMPL", "hip")


def _raw_fp8(a_q, a_s, b_q, b_s):
    return ops.hip_ext().gemm_bt_fp8(a_q, a_s, b_q, b_s)


def _raw_mx(a_q, a_s, b_q, b_s):
    return ops.hip_ext().gemm_bt_mxfp8(a_q, a_s, b_q, b_s)


# ---------------- fp8 128-tile kernel ----------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M,N", MN)
def test_fp8_gemm_bit_exact(dev, gen, hip_impl, M, N, K):
    for fn in (_raw_fp8, ops.gemm_bt_fp8):
        ko.check_qgemm_onehot(fn, "fp8", M, N, K, dev, gen)
        ko.check_qgemm_int(fn, "fp8", M, N, K, dev, gen)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M,N", MN)
def test_fp8_gemm_random(dev, gen, M, N, K):
    ko.check_qgemm_random(_raw_fp8, "fp8", M, N, K, dev, gen)


@pytest.mark.parametrize("K", [128, 640])
@pytest.mark.parametrize("M", M_PAD)
def test_fp8_gemm_padded_m(dev, gen, hip_impl, M, K):
    """ops pads A_q with zero rows and a_s with 1.0 up to the tile and
    returns exactly M rows (the shape is part of every check)."""
    ko.check_qgemm_onehot(ops.gemm_bt_fp8, "fp8", M, 384, K, dev, gen)
    ko.check_qgemm_int(ops.gemm_bt_fp8, "fp8", M, 384, K, dev, gen)
    ko.check_qgemm_random(ops.gemm_bt_fp8, "fp8", M, 384, K, dev, gen)


# ---------------- mxfp8 128-tile kernel ----------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M,N", MN)
def test_mxfp8_gemm_bit_exact(dev, gen, M, N, K):
    ko.check_qgemm_onehot(_raw_mx, "mx", M, N, K, dev, gen)
    ko.check_qgemm_int(_raw_mx, "mx", M, N, K, dev, gen)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M,N", MN)
def test_mxfp8_gemm_random(dev, gen, M, N, K):
    ko.check_qgemm_random(_raw_mx, "mx", M, N, K, dev, gen)


@pytest.mark.parametrize("K", [128, 640])
@pytest.mark.parametrize("M", M_PAD)
def test_mxfp8_gemm_padded_m(dev, gen, M, K):
    """ops pads A_q with zero rows and a_s with byte 127 (2^0)."""
    ko.check_qgemm_onehot(ops.gemm_bt_mxfp8, "mx", M, 384, K, dev, gen)
    ko.check_qgemm_int(ops.gemm_bt_mxfp8, "mx", M, 384, K, dev, gen)
    ko.check_qgemm_random(ops.gemm_bt_mxfp8, "mx", M, 384, K, dev, gen)


@pytest.mark.parametrize("K", [128, 384])
def test_mxfp8_gemm_just_under_the_256_threshold(dev, gen, K):
    """(2304, 4096): 144 256-tiles < 160 -> still the 128-tile kernel, at
    576 workgroups."""
    ko.check_qgemm_onehot(_raw_mx, "mx", 2304, 4096, K, dev, gen)
    ko.check_qgemm_int(_raw_mx, "mx", 2304, 4096, K, dev, gen)


# ---------------- mxfp8 256-tile kernel ----------------
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("M,N", [(2560, 4096), (2560, 4352)])   # 160 / 170 tiles (remainder 2)
def test_mxfp8_gemm_256_bit_exact(dev, gen, M, N, K):
    ko.check_qgemm_onehot(_raw_mx, "mx", M, N, K, dev, gen)
    ko.check_qgemm_int(_raw_mx, "mx", M, N, K, dev, gen)


def test_mxfp8_gemm_256_random(dev, gen):
    ko.check_qgemm_random(_raw_mx, "mx", 2560, 4352, 384, dev, gen)


# ---------------- grouped GEMM ----------------
@pytest.mark.parametrize("offsets", ["host", "device"])
@pytest.mark.parametrize("K", [64, 128, 192])                   # 64: one K-tile
@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("sizes", SIZES)
def test_grouped_gemm_kernel(dev, gen, hip_impl, sizes, N, K, offsets):
    """The in-repo grouped kernel through ops.grouped_gemm_bt: empty experts,
    segments of 1 / 127 / 128 / 129 / 300 rows, everything in the last
    expert, a 130-row first expert.  a_sorted has no spare rows: ops pads
    for the last tile's 128-row stage itself."""
    ko.check_grouped_gemm(ops.grouped_gemm_bt, sizes, N, K, dev, gen, offsets=offsets)


def test_grouped_gemm_one_expert_equals_dense(dev, gen, hip_impl):
    """One expert whose segment covers every row is the dense GEMM: the
    grouped kernel and gemm_bt_bf16_kernel (256 x 256 is 2 x 2 tiles of 128)
    run one pipeline body, the same operations in the same order, so the
    outputs are equal bit for bit.  K = 192: three K-tiles."""
    M, N, K = 256, 256, 192
    a = ko.rand_bf16(gen, M, K).to(dev)
    w = ko.rand_bf16(gen, 1, N, K).to(dev)
    got = ops.grouped_gemm_bt(a, w, [0, M])
    exp = ops.hip_ext().gemm_bt(a, w[0])
    assert tuple(got.shape) == (M, N)
    assert torch.equal(got, exp)


# ---------------- quantizers ----------------
@pytest.mark.parametrize("K", [8, 64, 2048, 2056, 4096])
@pytest.mark.parametrize("rows", [1, 3, 64])
def test_quant_fp8_exact(dev, gen, rows, K):
    ko.check_quant_fp8(ops.quant_fp8, rows, K, dev, gen)


@pytest.mark.parametrize("K", [32, 64, 8192, 8224])            # 8192: one block per thread
@pytest.mark.parametrize("rows", [1, 3, 64])
def test_quant_mxfp8_exact(dev, gen, rows, K):
    ko.check_quant_mxfp8(ops.quant_mxfp8, rows, K, dev, gen)


def test_quantizers_return_empty_for_no_rows(dev):
    """An empty grid is a launch error, so returning at all shows that
    nothing was launched."""
    x = torch.zeros(0, 64, dtype=torch.bfloat16, device=dev)
    q, s = ops.quant_fp8(x)
    assert tuple(q.shape) == (0, 64) and q.dtype == torch.uint8
    assert tuple(s.shape) == (0,) and s.dtype == torch.float32
    q, s = ops.quant_mxfp8(x)
    assert tuple(q.shape) == (0, 64) and q.dtype == torch.uint8
    assert tuple(s.shape) == (0, 2) and s.dtype == torch.uint8
    torch.cuda.synchronize()


# ---------------- moe_combine ----------------
@pytest.mark.parametrize("H", [8, 264, 2048, 2056])            # 264: 33 vectors; 2056: 257
@pytest.mark.parametrize("k", [1, 2, 3])
def test_moe_combine_exact(dev, gen, k, H):
    ko.check_moe_combine(ops.hip_ext().moe_combine, 7, k, H, dev, gen)


# ---------------- binding rejections ----------------
def test_quant_gemm_bindings_reject_mismatched_operands(dev):
    """The kernels index every operand from M, N, K (and E) alone, so the
    bindings must refuse operands of another size or layout.  Host-side
    checks; every mismatched operand is too LARGE, so nothing here could read
    out of bounds even if a check were missing."""
    ext = ops.hip_ext()
    M = N = K = 128
    u8 = dict(dtype=torch.uint8, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    aq, bq = torch.zeros(M, K, **u8), torch.zeros(N, K, **u8)
    a1, b1 = torch.ones(M, **f32), torch.ones(N, **f32)
    am, bm = torch.full((M, K // 32), 127, **u8), torch.full((N, K // 32), 127, **u8)
    wide = torch.zeros(M, 2 * K, **u8)[:, :K]                    # non-contiguous A_q
    assert not wide.is_contiguous()
    for bad in (lambda: ext.gemm_bt_fp8(aq, torch.ones(M + 4, **f32), bq, b1),
                lambda: ext.gemm_bt_fp8(aq, a1, bq, torch.ones(N + 4, **f32)),
                lambda: ext.gemm_bt_fp8(wide, a1, bq, b1),
                lambda: ext.gemm_bt_mxfp8(aq, torch.full((M + 4, K // 32), 127, **u8), bq, bm),
                lambda: ext.gemm_bt_mxfp8(aq, am, bq, torch.full((N + 4, K // 32), 127, **u8)),
                lambda: ext.gemm_bt_mxfp8(aq, torch.full((M, K // 32 + 1), 127, **u8), bq, bm),
                lambda: ext.gemm_bt_mxfp8(aq, am, bq, torch.full((N, K // 32 + 1), 127, **u8)),
                lambda: ext.gemm_bt_mxfp8(wide, am, bq, bm)):
        with pytest.raises(RuntimeError):
            bad()
    assert tuple(ext.gemm_bt_fp8(aq, a1, bq, b1).shape) == (M, N)      # the well-formed call
    assert tuple(ext.gemm_bt_mxfp8(aq, am, bq, bm).shape) == (M, N)

    bf = dict(dtype=torch.bfloat16, device=dev)
    a, w = torch.zeros(256, 64, **bf), torch.zeros(2, 128, 64, **bf)

    def i32(v):
        return torch.tensor(v, dtype=torch.int32, device=dev)

    te, tm, ends = i32([0, 1]), i32([0, 128]), i32([128, 256])
    with pytest.raises(RuntimeError):                                  # E + 1 segment ends
        ext.grouped_gemm_bt(a, w, te, tm, i32([128, 256, 256]))
    with pytest.raises(RuntimeError):                                  # a tile start too many
        ext.grouped_gemm_bt(a, w, te, i32([0, 128, 128]), ends)
    with pytest.raises(RuntimeError):                                  # non-contiguous A
        ext.grouped_gemm_bt(torch.zeros(256, 128, **bf)[:, :64], w, te, tm, ends)
    assert tuple(ext.grouped_gemm_bt(a, w, te, tm, ends).shape) == (256, 128)
    torch.cuda.synchronize()
