"""Packed attention reading V from the qkv rows: attn_fwd_v5_packed_rm_qkv
must write, bit for bit, what attn_fwd_v5_packed_rm writes from the V^T that
vt_from_qkv_packed makes of the same qkv — the same MFMA operands in the same
order, fetched by another route — and nothing else.

The kernel bindings are called directly (the op-level dispatch sends grids
this small to v2).  Shapes and skips are those of test_attn_rowmajor_gpu.py:
S = 384 has the inert upper waves of a 256-row block, S = 640 a third block;
the skips fall inside a block (64, 192), exactly on one (256) and past one
(320).  'diffuse' keeps defer-max on, 'early_spike' breaks it once and
'stair+9' climbs 9 nats per tile, past the 8-nat threshold, so every tile
rescales O: the three paths a tile above a wave's rows passes through.

qkv is [lead + Tp + tail, ld] with ld 8 columns wider than the heads: the
rows before and after the plan's, and the pad columns, are NaN, so a V read
from outside the plan poisons the output.  The output buffer is pre-filled
with a sentinel at the same rows, which must keep it.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_oracles as ko
import model_oracle as mo
from senweaver_amd import ops
from senweaver_amd.engine.prefix_plan import plan_from_skips, plan_from_tokens

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


def _packed_qkv(gen, v, plan, H, Hk, lead, tail):
    """[lead + Tp + tail, (H + 2Hk)*D + 8]: random q/k filler, the V slice of
    packed row base[b] + s from v[b, :, s]; everything else NaN."""
    cols = (H + 2 * Hk) * D
    qkv = torch.full((lead + plan.Tp + tail, cols + 8), float("nan"), dtype=ko.BF16)
    qkv[lead:lead + plan.Tp, :(H + Hk) * D] = ko.rand_bf16(gen, plan.Tp, (H + Hk) * D)
    for b in range(plan.B):
        s0 = plan.skip[b]
        r0 = lead + plan.base[b] + s0
        qkv[r0:r0 + plan.S - s0, (H + Hk) * D:cols] = \
            v[b, :, s0:].permute(1, 0, 2).reshape(plan.S - s0, Hk * D)
    return qkv


def _check(dev, c, H, Hk, plan, gen, what):
    ext = ops.hip_ext()
    B, S = plan.B, plan.S
    q, k = c["q"].to(dev), c["k"].to(dev)
    # the bindings take at most B*S rows: a plan with nothing shared has no
    # room for sentinel rows
    lead, tail = (LEAD, TAIL) if plan.Tp + LEAD + TAIL <= B * S else (0, 0)
    rows = lead + plan.Tp + tail
    qkv = _packed_qkv(gen, c["v"], plan, H, Hk, lead, tail).to(dev)
    d_skip = torch.tensor(plan.skip, dtype=torch.int32, device=dev)
    d_base = torch.tensor([b + lead for b in plan.base], dtype=torch.int32, device=dev)
    d_owner = torch.tensor(plan.owner, dtype=torch.int32, device=dev)
    vt = ext.vt_from_qkv_packed(qkv, H, Hk, D, B, S, d_skip, d_base, d_owner)
    exp = ext.attn_fwd_v5_packed_rm(q, k, vt, c["scale"], d_skip, d_base, rows)
    out = torch.full((rows, H * D), ko.SENTINEL, dtype=ko.BF16, device=dev)
    got = ext.attn_fwd_v5_packed_rm_qkv(q, k, qkv, H, Hk, c["scale"], d_skip,
                                        d_base, d_owner, rows, out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (rows, H * D)
    written = slice(lead, lead + plan.Tp)
    assert not torch.isnan(exp[written].float()).any(), what + ": the reference read a NaN row"
    ko.assert_bits_equal(got[written].contiguous(), exp[written].contiguous(), what)
    sentinel = torch.full((lead + tail, H * D), ko.SENTINEL, dtype=ko.BF16)
    ko.assert_bits_equal(torch.cat([got[:lead], got[lead + plan.Tp:]]), sentinel,
                         what + " rows outside the plan")
    fresh = ext.attn_fwd_v5_packed_rm_qkv(q, k, qkv, H, Hk, c["scale"], d_skip,
                                          d_base, d_owner, rows)
    ko.assert_bits_equal(fresh[written].contiguous(), got[written].contiguous(),
                         what + " own buffer")


def _modes(S):
    return ("diffuse", "early_spike", "stair+9") if S == 640 else ("diffuse",)


@pytest.mark.parametrize("B,H,Hk", [(2, 2, 1), (3, 6, 2)])
@pytest.mark.parametrize("S", [256, 384, 640])
def test_v_rows_match_the_transposed_route(dev, S, B, H, Hk):
    for mode in _modes(S):
        gen = torch.Generator().manual_seed(9400 + S)
        c = ko.make_prefill_case(gen, mode, B, H, Hk, S)
        for skips in _skip_rows(B, S):
            plan = plan_from_skips((0,) * B, skips, S)
            _check(dev, c, H, Hk, plan, gen,
                   f"{mode} S={S} B={B} H={H} Hk={Hk} skips={skips}")


def test_two_groups_leader_not_row_zero(dev):
    """owner = (0, 0, 2, 2): rows 2 and 3 take their prefix from row 2."""
    B, H, Hk, S = 4, 2, 1, 384
    gen = torch.Generator().manual_seed(9477)
    c = ko.make_prefill_case(gen, "diffuse", B, H, Hk, S)
    for skips in [(0, 64, 0, 192), (0, 320, 0, 256)]:
        plan = plan_from_skips((0, 0, 2, 2), skips, S)
        _check(dev, c, H, Hk, plan, gen, f"two groups S={S} skips={skips}")


def test_prefill_packed_same_bits_with_and_without_the_v_rows_route(dev, monkeypatch):
    """LlamaModel.prefill_packed, 2 layers, S = 256, at a shape whose grid
    does reach v5 (16 rows x 32 heads = 512 blocks): the route through
    attn_fwd_v5_packed_rm_qkv against vt_from_qkv_packed +
    attn_fwd_v5_packed_rm, the route it replaced."""
    B, S = 16, 256
    model = mo.build_model(mo.cfg_small(heads=32, kv_heads=8), "bf16", dev)
    tokens = mo.dense_tokens(B, S, seed=31)
    # groups of four: members share 200, 128 and 64 tokens with their leader
    # (descending, because a plan never shares more than the row before did)
    for b in range(B):
        shared = (0, 200, 128, 64)[b % 4]
        tokens[b, :shared] = tokens[b - b % 4, :shared]
    plan = plan_from_tokens(tokens.tolist())
    assert not plan.is_identity and plan.skip[:4] == (0, 192, 128, 64)

    called = set()
    ext = ops.hip_ext()

    class Spy:
        def __getattr__(self, name):
            called.add(name)
            return getattr(ext, name)

    monkeypatch.setattr(ops, "hip_ext", lambda: Spy())
    new = model.prefill_packed(tokens.to(dev), plan)
    assert "attn_fwd_v5_packed_rm_qkv" in called and "vt_from_qkv_packed" not in called

    def old_route(qb, kb, qkv, Hq, Hk, D_, scale, skip, base, owner, Tp, flat_idx):
        vt = ops.vt_from_qkv_packed(qkv, Hq, Hk, D_, qb.shape[0], qb.shape[2],
                                    skip, base, owner)
        return ops.attn_fwd_packed(qb, kb, vt, scale, skip, base, Tp, flat_idx)

    called.clear()
    monkeypatch.setattr(ops, "attn_fwd_packed_qkv", old_route)
    old = model.prefill_packed(tokens.to(dev), plan)
    assert {"vt_from_qkv_packed", "attn_fwd_v5_packed_rm"} <= called
    assert "attn_fwd_v5_packed_rm_qkv" not in called
    ko.assert_bits_equal(new, old, "prefill_packed B=16 H=32 Hk=8 S=256")
