"""Prefix-packed prefill on the GPU.

Kernel checks are BIT-EQUAL against the unpacked kernels: per-row math is
unchanged, only addresses move.
  * rope_scatter_qkv_packed / vt_from_qkv_packed on a packed qkv against
    rope_scatter_qkv / vt_from_qkv on the unpacked tensor it was packed from;
  * attn_fwd_v5_packed: EVERY one of the Tp columns of the packed O^T against
    the matching column of attn_fwd_v5 on the same Q/K/V^T (all columns, so a
    misplaced store shows), with skips on a wave edge inside block 0, on a
    block edge, a block plus a straddle, and S - 64, at S with dead upper
    waves in the last 256-row block, GQA ratios 2 and 3.
Model-level checks (tiny-debug, B=4, S=256, prefix 200) use the measured
tolerance of tests/prefix_pack_cases.py.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_oracles as ko
import prefix_pack_cases as pc
from senweaver_amd import ops
from senweaver_amd.engine.prefix_plan import plan_from_skips
from senweaver_amd.engine.scorer import LlamaBackend
from senweaver_amd.models.config import get_config
from senweaver_amd.models.llama import LlamaModel
from senweaver_amd.ops import reference as ref

D = 128


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_loaded(), "HIP extension failed to build/load"
    return torch.device("cuda:0")


@pytest.fixture
def gen():
    return torch.Generator().manual_seed(20251)


def _plan_dev(plan, dev):
    return tuple(torch.tensor(x, dtype=torch.int32, device=dev)
                 for x in (plan.skip, plan.base, plan.owner))


# ---------------- rope_scatter and V^T ----------------
@pytest.mark.parametrize("B,Hq,Hk,S,owner,skip", [
    (3, 2, 1, 256, (0, 0, 0), (0, 64, 192)),
    (4, 6, 2, 384, (0, 0, 2, 2), (0, 128, 0, 320)),
])
def test_rope_scatter_and_vt_packed_bit_equal(dev, gen, B, Hq, Hk, S, owner, skip):
    ext = ops.hip_ext()
    plan = plan_from_skips(owner, skip, S)
    ld = (Hq + 2 * Hk) * D
    qkv = ko.rand_bf16(gen, B, S, ld)
    for b in range(B):           # member prefixes are copies of the leader's
        qkv[b, :skip[b]] = qkv[owner[b], :skip[b]]
    qkv = qkv.reshape(B * S, ld)
    stored = torch.tensor([b * S + s for b, s in plan.stored_tokens()])
    packed = qkv[stored].contiguous()
    assert packed.shape[0] == plan.Tp < B * S
    cos_sin = ops.rope_tables(512, D).to(dev)
    pos = torch.arange(S, dtype=torch.int32).repeat(B)
    d_skip, d_base, d_owner = _plan_dev(plan, dev)

    q_exp, k_exp = ext.rope_scatter_qkv(qkv.to(dev), cos_sin, pos.to(dev),
                                        Hq, Hk, D, B, S)
    q_got, k_got = ext.rope_scatter_qkv_packed(
        packed.to(dev), cos_sin, pos[stored].to(dev), Hq, Hk, D, B, S,
        d_skip, d_base, d_owner)
    ko.assert_bits_equal(q_got, q_exp, "rope_scatter_qkv_packed Q")
    ko.assert_bits_equal(k_got, k_exp, "rope_scatter_qkv_packed K")

    vt_exp = ext.vt_from_qkv(qkv.to(dev), Hq, Hk, D, B, S)
    vt_got = ext.vt_from_qkv_packed(packed.to(dev), Hq, Hk, D, B, S,
                                    d_skip, d_base, d_owner)
    ko.assert_bits_equal(vt_got, vt_exp, "vt_from_qkv_packed")


# ---------------- attention ----------------
ATTN_SKIPS = [64, 192, 256, 320]
ATTN_CASES = sorted({(S, sk) for S in (256, 384, 640)
                     for sk in ATTN_SKIPS + [S - 64] if sk <= S - 64})


@pytest.mark.parametrize("B,H,Hk", [(2, 4, 2), (2, 6, 2)])
@pytest.mark.parametrize("S,skip1", ATTN_CASES)
def test_attn_packed_every_column_bit_equal(dev, gen, S, skip1, B, H, Hk):
    ext = ops.hip_ext()
    plan = plan_from_skips((0, 0), (0, skip1), S)
    c = ko.make_prefill_case(gen, "diffuse", B, H, Hk, S)
    q, k, vt = c["q"].to(dev), c["k"].to(dev), c["vt"].to(dev)
    d_skip, d_base, _ = _plan_dev(plan, dev)
    full = ext.attn_fwd_v5(q, k, vt, c["scale"])          # [B,H,D,S]
    got = ext.attn_fwd_v5_packed(q, k, vt, c["scale"], d_skip, d_base, plan.Tp)
    assert tuple(got.shape) == (H * D, plan.Tp)
    exp = ref.pack_ot_ref(full, d_skip, d_base, plan.Tp)
    ko.assert_bits_equal(got, exp, f"attn packed S={S} skip={skip1} H={H} Hk={Hk}")


# ---------------- swiglu into a row-padded buffer ----------------
@pytest.mark.parametrize("rows,out_rows,inter", [(192, 256, 512), (65, 65, 264), (3, 130, 2056)])
def test_swiglu_padded_bit_equal_and_zero_tail(dev, gen, rows, out_rows, inter):
    ext = ops.hip_ext()
    gateup = ko.rand_bf16(gen, rows, 2 * inter).to(dev)
    got = ext.swiglu_padded(gateup, out_rows)
    assert tuple(got.shape) == (out_rows, inter)
    ko.assert_bits_equal(got[:rows], ext.swiglu(gateup), "swiglu_padded rows")
    ko.assert_bits_equal(got[rows:], torch.zeros(out_rows - rows, inter, dtype=ko.BF16),
                         "swiglu_padded tail")
    ko.assert_bits_equal(ops.swiglu(gateup, out_rows), got, "ops.swiglu(out_rows)")


# ---------------- model level ----------------
@pytest.fixture(scope="module")
def tiny_tokens():
    return pc.shared_prefix_tokens(4, 256, 200, get_config("tiny-debug").vocab_size)


def test_prefill_packed_matches_prefill_gpu(dev, tiny_tokens):
    model = LlamaModel(get_config("tiny-debug"), device=dev, seed=0)
    plan = pc.check_prefill_packed(model, tiny_tokens)
    assert plan.skip == (0, 192, 192, 192)


def test_scorer_prefix_pack_switch_gpu(dev, tiny_tokens):
    mask = torch.zeros(4, 256, dtype=torch.bool)
    mask[:, 150:180] = True
    mask[:, 190:230] = True
    mask[2, 255] = True

    def make(pack):
        return LlamaBackend("tiny-debug", device="cuda:0", seed=0, max_seq=256,
                            micro_batch=4, prefix_pack=pack)

    pc.check_scorer(make, tiny_tokens, mask)
