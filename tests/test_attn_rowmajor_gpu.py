"""Row-major O from the packed attention kernel: attn_fwd_v5_packed_rm must
write, bit for bit, the transpose of attn_fwd_v5_packed's O^T — the same
values at another address — and nothing else.

The kernel bindings are called directly (the op-level dispatch sends grids
this small to v2).  S = 384 has the inert upper waves of a 256-row block;
the skips fall inside a block (64, 192), exactly on one (256) and past one
(320); skip 0 everywhere is a plan with nothing shared.  The output buffer
is pre-filled with a sentinel and is longer than the plan at both ends:
rows outside every [base, base + S - skip) must keep it.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_oracles as ko
from senweaver_amd import ops
from senweaver_amd.engine.prefix_plan import plan_from_skips

D = 128
SKIPS = [0, 64, 192, 256, 320]
LEAD, TAIL = 5, 3   # sentinel rows before and after the plan's rows


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_loaded(), "HIP extension failed to build/load"
    return torch.device("cuda:0")


def _skip_rows(B, S):
    """Per-row skips (row 0 leads): every legal value in turn for row 1, the
    next one along for row 2."""
    legal = [s for s in SKIPS if s <= S - 64]
    for i, sk in enumerate(legal):
        yield (0, sk) if B == 2 else (0, sk, legal[(i + 1) % len(legal)])


@pytest.mark.parametrize("B,H,Hk", [(2, 2, 1), (3, 6, 2)])
@pytest.mark.parametrize("S", [256, 384, 640])
def test_rowmajor_is_the_transpose_and_touches_nothing_else(dev, S, B, H, Hk):
    ext = ops.hip_ext()
    gen = torch.Generator().manual_seed(9300 + S)
    c = ko.make_prefill_case(gen, "diffuse", B, H, Hk, S)
    q, k, vt = c["q"].to(dev), c["k"].to(dev), c["vt"].to(dev)
    for skips in _skip_rows(B, S):
        plan = plan_from_skips((0,) * B, skips, S)
        # the bindings take Tp <= B*S: a plan with nothing shared has no
        # room for sentinel rows
        lead, tail = (LEAD, TAIL) if plan.Tp + LEAD + TAIL <= B * S else (0, 0)
        rows = lead + plan.Tp + tail
        d_skip = torch.tensor(plan.skip, dtype=torch.int32, device=dev)
        d_base = torch.tensor([b + lead for b in plan.base], dtype=torch.int32, device=dev)
        ot = ext.attn_fwd_v5_packed(q, k, vt, c["scale"], d_skip, d_base, rows)
        out = torch.full((rows, H * D), ko.SENTINEL, dtype=ko.BF16, device=dev)
        got = ext.attn_fwd_v5_packed_rm(q, k, vt, c["scale"], d_skip, d_base, rows, out)
        assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (rows, H * D)
        what = f"S={S} B={B} H={H} Hk={Hk} skips={skips}"
        written = slice(lead, lead + plan.Tp)
        ko.assert_bits_equal(got[written], ot.t()[written].contiguous(), what)
        sentinel = torch.full((lead + tail, H * D), ko.SENTINEL, dtype=ko.BF16)
        ko.assert_bits_equal(torch.cat([got[:lead], got[lead + plan.Tp:]]), sentinel,
                             what + " rows outside the plan")
        fresh = ext.attn_fwd_v5_packed_rm(q, k, vt, c["scale"], d_skip, d_base, rows)
        ko.assert_bits_equal(fresh[written], got[written].contiguous(), what + " own buffer")
