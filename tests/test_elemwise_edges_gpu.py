"""Exactness tests for the elementwise kernels on the GPU — add_bf16,
rmsnorm, fused_add_rmsnorm, swiglu / swiglu_padded and rope_inplace — against
the fp64 oracles in tests/kernel_oracles.py.

Shapes are the smallest that reach each loop shape of a 256-thread block of
8-element vectors: hidden / inter = 8 (one thread), 2040 (a partial pass),
2048 (exactly one pass), 2056 (thread 0 takes a second vector); add_bf16 at
one vector, at exactly the 2048-block grid cap and one vector past it (the
grid-stride loop's second trip); rope at D = 32 (a quarter wave), 128 and 256
(two trips of the 64-thread loop).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_oracles as ko
from senweaver_amd import ops
from senweaver_amd.ops import reference as ref

HIDDEN = [8, 2040, 2048, 2056]
ROWS = [1, 3]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_loaded(), "HIP extension failed to build/load"
    return torch.device("cuda:0")


@pytest.fixture
def gen():
    return torch.Generator().manual_seed(33119)


def _fused(x, res, w, eps):
    y = ops.fused_add_rmsnorm(x, res, w, eps)      # res updated in place
    return y, res


def _swiglu_padded(gu, out_rows):
    return ops.hip_ext().swiglu_padded(gu, out_rows)


@pytest.mark.parametrize("n", [8, 8 * 256 * 2048, 8 * 256 * 2048 + 8])
def test_add_bf16_exact(dev, gen, n):
    ko.check_add_bf16(ops.hip_ext().add_bf16, n, dev, gen)


@pytest.mark.parametrize("hidden", HIDDEN)
@pytest.mark.parametrize("rows", ROWS)
def test_rmsnorm_exact(dev, gen, rows, hidden):
    ko.check_rmsnorm(ops.rmsnorm, rows, hidden, dev, gen)


@pytest.mark.parametrize("hidden", HIDDEN)
@pytest.mark.parametrize("rows", ROWS)
def test_fused_add_rmsnorm_exact(dev, gen, rows, hidden):
    ko.check_fused_add_rmsnorm(_fused, rows, hidden, dev, gen)


@pytest.mark.parametrize("inter", [8, 2040, 2056])
@pytest.mark.parametrize("rows", [0, 1, 3])
def test_swiglu_and_padded(dev, gen, rows, inter):
    """swiglu against fp64; swiglu_padded at out_rows = rows, rows + 1 and
    rows + 3 (and with no input rows at all): head bit-equal, pad rows +0."""
    ko.check_swiglu(ops.swiglu, _swiglu_padded, rows, inter, dev, gen)
    if rows:      # the ops wrapper takes the padded kernel only past the input's rows
        gu = ko.swiglu_inputs(gen, rows, inter).to(dev)
        y = ops.swiglu(gu, out_rows=rows + 2)
        assert tuple(y.shape) == (rows + 2, inter)
        ko.assert_bits_equal(y[:rows].contiguous(), ops.swiglu(gu), "ops.swiglu out_rows")


@pytest.mark.parametrize("Hq,Hk", [(1, 1), (6, 2)])
@pytest.mark.parametrize("D", [32, 128, 256])
def test_rope_inplace_exact(dev, gen, D, Hq, Hk):
    ko.check_rope_inplace(ops.rope_inplace, Hq, Hk, D, dev, gen, ref.rope_tables)


def test_elementwise_bindings_reject_mismatched_operands(dev):
    """Host-side checks.  Every bad operand is too LARGE, of a size the
    kernel would still read in bounds, or on the CPU, so nothing here could
    read out of bounds even if a check were missing."""
    ext = ops.hip_ext()
    bf = dict(dtype=torch.bfloat16, device=dev)
    x, res, w = torch.zeros(2, 64, **bf), torch.zeros(2, 64, **bf), torch.ones(64, **bf)
    w_long = torch.ones(72, **bf)
    x12, res12, w12 = torch.zeros(2, 12, **bf), torch.zeros(2, 12, **bf), torch.ones(12, **bf)
    for bad in (lambda: ext.rmsnorm(x, w_long, 1e-5),
                lambda: ext.rmsnorm(x, w.cpu(), 1e-5),
                lambda: ext.rmsnorm(x12, w12, 1e-5),
                lambda: ext.fused_add_rmsnorm(x, res, w_long, 1e-5),
                lambda: ext.fused_add_rmsnorm(x, torch.zeros(3, 64, **bf), w, 1e-5),
                lambda: ext.fused_add_rmsnorm(x, torch.zeros(2, 128, **bf), w, 1e-5),
                lambda: ext.fused_add_rmsnorm(x, res.cpu(), w, 1e-5),
                lambda: ext.fused_add_rmsnorm(x12, res12, w12, 1e-5)):
        with pytest.raises(RuntimeError):
            bad()
    assert tuple(ext.rmsnorm(x, w, 1e-5).shape) == (2, 64)          # the well-formed calls
    assert tuple(ext.fused_add_rmsnorm(x, res, w, 1e-5).shape) == (2, 64)

    T, D = 3, 32
    q, k = torch.zeros(T, 2, D, **bf), torch.zeros(T, 1, D, **bf)
    cs = ref.rope_tables(16, D).to(dev)
    pos = torch.zeros(T, dtype=torch.int32, device=dev)
    for bad in (lambda: ext.rope_inplace(q, k, cs, torch.zeros(T + 1, dtype=torch.int32, device=dev)),
                lambda: ext.rope_inplace(q, k, cs, pos.cpu()),
                lambda: ext.rope_inplace(q, k, cs.cpu(), pos),
                lambda: ext.rope_inplace(q, k.cpu(), cs, pos),
                lambda: ext.rope_inplace(q, torch.zeros(T + 1, 1, D, **bf), cs, pos)):
        with pytest.raises(RuntimeError):
            bad()
    ext.rope_inplace(q, k, cs, pos)
    torch.cuda.synchronize()
