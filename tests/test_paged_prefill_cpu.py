"""ops.paged_prefill_attn on the CPU (the fp32 reference) under the same
drivers as the GPU kernel (tests/paged_prefill_cases.py), on the small
cases: the reference is built row by row and is slow at the large ones."""

import pytest
import torch

import kernel_oracles as ko
import paged_prefill_cases as pp
from senweaver_amd import ops

DEV = torch.device("cpu")
SMALL = [(64, 64), (80, 16), (100, 1), (150, 5), (200, 17)]


@pytest.fixture
def gen():
    return torch.Generator().manual_seed(20251)


def test_scatter_construction_agrees_with_decode_oracle(gen):
    pp.check_scatter_agrees(gen)


@pytest.mark.parametrize("tmap", ["diag", "tile_prev_last", "random"])
@pytest.mark.parametrize("ctx,q_len", SMALL[1:])
def test_pointer_bit_exact(gen, ctx, q_len, tmap):
    pp.check_pointer(ops.paged_prefill_attn, DEV, gen, ctx, q_len, tmap)


@pytest.mark.parametrize("ctx,q_len", [(80, 16), (150, 5)])
def test_future_decoy_is_masked(gen, ctx, q_len):
    pp.check_future_decoy(ops.paged_prefill_attn, DEV, gen, ctx, q_len)


def test_random_vs_fp64_and_pad_rows(gen):
    pp.check_random(ops.paged_prefill_attn, DEV, gen, [(100, 1), (150, 5)], 4, 2)
    pp.check_pad_and_stale(ops.paged_prefill_attn, DEV, gen, [(80, 16), (150, 5)], 4, 2)


def test_default_scale_and_length_contract(gen):
    c = pp.make_random_case(gen, [(80, 16)], 2, 1)
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32)
    a = ops.paged_prefill_attn(c["q"], c["kcache"], c["vcache"], c["block_table"],
                               i32([80]), i32([16]))
    b = ops.paged_prefill_attn(c["q"], c["kcache"], c["vcache"], c["block_table"],
                               i32([80]), i32([16]), c["scale"])
    ko.assert_bits_equal(a, b, "default scale")
    with pytest.raises(AssertionError):   # q_len > Sq
        ops.paged_prefill_attn(c["q"], c["kcache"], c["vcache"], c["block_table"],
                               i32([80]), i32([17]))
