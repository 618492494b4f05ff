"""Exactness tests for the dense bf16 GEMM kernels on the GPU, each against
the CPU oracles in tests/kernel_oracles.py:

  * gemm_bt_bf16_8ph_v14_kernel, gemm_bt_bf16_asm4_kernel and
    gemm_bt_bf16_asm7_kernel (the 256-tile kernels gemm_bt dispatches to),
    run directly through gemm_bt_8ph_v;
  * gemm_bt_bf16_kernel (128-tile) and gemm_bt_bf16_256_kernel through gemm_bt;
  * the dispatch of gemm_bt on both sides of each of its thresholds;
  * the M pad of ops.gemm_bt_tiled and the operand checks of the bindings.

Three checks per shape (derivations in kernel_oracles): one-hot in K on A and
on B -> bit-exact; small integers over all of K -> bit-exact; randn against
the fp64 product within 2^-8 |ref| + K 2^-24 |A|.|B|^T.

Every kernel here walks K in tiles of 64, so K = 128 .. 640 is 2 .. 10 tiles:
both parities of the A double buffer, three laps of the B ring of three, and
the shortest K the pipelined kernels accept (prologue straight into the drain
of the last two tiles).  Grids: 1 workgroup; 3 x 5 = 15 (XCD remainder 7);
9 x 3 = 27 (remainder 3, last grouped-m block one tile high); 12 x 2 (last
block four high); 16 x 1 (two full blocks of one column).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_oracles as ko
from senweaver_amd import ops

VARS = [14, 21, 24]                                   # v14, asm4, asm7
K256 = [128, 256, 384, 512, 640]
GRID_K = [(1, 1), (3, 5)]                             # 256-tiles (m, n)
GRID_384 = [(9, 3), (12, 2), (16, 1)]
K128 = [64, 128, 192, 320]                            # 64: a single K-tile
GRID_128 = [(1, 1), (2, 3), (3, 3), (4, 5)]           # 128-tiles (m, n)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_loaded(), "HIP extension failed to build/load"
    return torch.device("cuda:0")


@pytest.fixture
def gen():
    return torch.Generator().manual_seed(50917)


@pytest.fixture
def hip_impl(monkeypatch):
    """ops.* routes to the in-repo kernels, as SENWEAVER_GEMM=hip does."""
    monkeypatch.setattr(ops, "_GEMM_IMPL", "hip")


def _variant(var):
    return lambda a, b: ops.hip_ext().gemm_bt_8ph_v(a, b, var)


def _raw(a, b):
    return ops.hip_ext().gemm_bt(a, b)


# ---------------- 256-tile kernels, run directly ----------------
@pytest.mark.parametrize("K", K256)
@pytest.mark.parametrize("tm,tn", GRID_K)
@pytest.mark.parametrize("var", VARS)
def test_gemm_256_k_sweep(dev, gen, var, tm, tn, K):
    ko.check_gemm_all(_variant(var), 256 * tm, 256 * tn, K, dev, gen)


@pytest.mark.parametrize("tm,tn", GRID_384)
@pytest.mark.parametrize("var", VARS)
def test_gemm_256_grid_sweep(dev, gen, var, tm, tn):
    ko.check_gemm_all(_variant(var), 256 * tm, 256 * tn, 384, dev, gen)


# ---------------- 128-tile kernel ----------------
@pytest.mark.parametrize("K", K128)
@pytest.mark.parametrize("tm,tn", GRID_128)
def test_gemm_128_kernel(dev, gen, tm, tn, K):
    """Through gemm_bt: 1, 6, 9 and 20 workgroups, far below the 160
    256-tiles at which the dispatch leaves the 128-tile kernel."""
    ko.check_gemm_all(_raw, 128 * tm, 128 * tn, K, dev, gen)


# ---------------- gemm_bt dispatch boundaries ----------------
DISPATCH = [
    # 159 | 160 256-tiles: 128-tile kernel at 636 workgroups | v14
    (768, 13568, 128), (2560, 4096, 128), (2560, 4096, 256),
    # M 3840 | 4096, at least 160 tiles on both sides: v14 | asm4
    (3840, 2816, 128), (4096, 2560, 128), (4096, 2560, 256),
    # M 7936 | 8192: asm4 at 31 x 6 tiles | asm7 at 32 x 5
    (7936, 1536, 128), (8192, 1280, 128), (8192, 1280, 256),
    # wide-N rule 2N >= 7M.  At two m-tiles both sides of it (N = 1792 | 1536)
    # have 14 and 12 256-tiles, under the 160 the 256-tile kernels need, so the
    # 128-tile kernel serves both; the rule first switches kernels at eight
    # m-tiles: N = 7168 (asm7) | 6912 (v14)
    (512, 1792, 128), (512, 1536, 128), (2048, 7168, 128), (2048, 6912, 128),
    # K % 128 != 0 at 160 tiles: gemm_bt_bf16_256_kernel
    (2560, 4096, 192),
]


@pytest.mark.parametrize("M,N,K", DISPATCH)
def test_gemm_bt_dispatch_boundaries(dev, gen, M, N, K):
    """The same three checks whichever kernel gemm_bt picks for the shape."""
    ko.check_gemm_all(_raw, M, N, K, dev, gen)


@pytest.mark.parametrize("K", [64, 192, 320])
def test_gemm_256_drain_kernel_k_sweep(dev, gen, K):
    """gemm_bt_bf16_256_kernel (full drain per K-tile) is what gemm_bt runs at
    160 tiles when K is no multiple of 128: one, three and five K-tiles."""
    ko.check_gemm_all(_raw, 2560, 4096, K, dev, gen)


# ---------------- ops: M pad and operand views ----------------
@pytest.mark.parametrize("M,N,K", [(17, 256, 192), (129, 256, 192), (300, 256, 192),
                                   (2305, 4096, 128), (2305, 4096, 192)])
def test_gemm_ops_pad_m(dev, gen, hip_impl, M, N, K):
    """ops pads M to 128 (N = 256) or to the 256-tile (2305 -> 2560 at N =
    4096: 160 tiles) and returns exactly M rows; the row count is part of
    every check."""
    for fn in (ops.gemm_bt_tiled, ops.gemm_bt):
        ko.check_gemm_onehot(fn, M, N, K, dev, gen)
        ko.check_gemm_int(fn, M, N, K, dev, gen)
        ko.check_gemm_random(fn, M, N, K, dev, gen)


@pytest.mark.parametrize("M", [300, 256])            # padded and unpadded
def test_gemm_ops_noncontiguous_views(dev, gen, hip_impl, M):
    """a as a transposed view and b as a column slice give the bits of their
    contiguous copies, which are the exact integer product."""
    N, K = 256, 192
    a, b = ko.gemm_int_operands(gen, M, N, K)
    exp = ko.exact_bf16((a.float() @ b.float().t()).double())
    a_t = a.t().contiguous().to(dev).t()                                   # [M, K], stride (1, M)
    b_s = torch.cat([b, ko.rand_bf16(gen, N, K)], dim=1).to(dev)[:, :K]    # stride (2K, 1)
    assert not a_t.is_contiguous() and not b_s.is_contiguous()
    for fn in (ops.gemm_bt_tiled, ops.gemm_bt):
        ko.assert_bits_equal(fn(a_t, b_s), exp, f"views M={M}")
        ko.assert_bits_equal(fn(a_t.contiguous(), b_s.contiguous()), exp, f"copies M={M}")


# ---------------- binding rejections ----------------
def test_gemm_bindings_reject_mismatched_operands(dev):
    """The kernels index both operands from M, N and K alone.  Host-side
    checks; every bad operand is too LARGE or on the CPU, so nothing here
    could read out of bounds even if a check were missing."""
    ext = ops.hip_ext()
    bf = dict(dtype=torch.bfloat16, device=dev)
    a, b = torch.zeros(256, 128, **bf), torch.zeros(256, 128, **bf)
    b_wide = torch.zeros(256, 256, **bf)                    # another K
    a3, b3 = torch.zeros(256, 128, 2, **bf), torch.zeros(256, 128, 2, **bf)
    b_cpu = torch.zeros(256, 128, dtype=torch.bfloat16)
    two = {"gemm_bt": ext.gemm_bt,
           "gemm_bt_8ph_v": lambda x, y: ext.gemm_bt_8ph_v(x, y, 14)}
    for name, fn in two.items():
        for bad in ((a, b_wide), (a3, b), (a, b3), (a, b_cpu), (b_cpu, b)):
            with pytest.raises(RuntimeError):
                fn(*bad)
        assert tuple(fn(a, b).shape) == (256, 256), name    # the well-formed call
    for var in (-1, 0, 10, 13, 15, 18, 25, 1000):           # no such variant
        with pytest.raises(RuntimeError):
            ext.gemm_bt_8ph_v(a, b, var)
    for var in (14, 21, 24):
        assert tuple(ext.gemm_bt_8ph_v(a, b, var).shape) == (256, 256)
    # K below the two tiles the pipelined prologues need; K = 0
    a64, b64 = torch.zeros(256, 64, **bf), torch.zeros(256, 64, **bf)
    a0, b0 = torch.zeros(256, 0, **bf), torch.zeros(256, 0, **bf)
    for bad in ((a64, b64), (a0, b0)):
        with pytest.raises(RuntimeError):
            two["gemm_bt_8ph_v"](*bad)
    with pytest.raises(RuntimeError):
        ext.gemm_bt(a0, b0)
    assert tuple(ext.gemm_bt(a64, b64).shape) == (256, 256)
    torch.cuda.synchronize()
