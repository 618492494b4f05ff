"""Exactness tests for the prefill attention kernels on the GPU: the 64-row
attn_fwd (v1), attn_fwd_v2, attn_fwd_v3 and the production attn_fwd_v5, the
ops.attn_fwd_t / ops.attn_fwd dispatch around them, the bindings' shape
checks and the vt_from_qkv transpose that feeds them.  Oracles, generators
and the error bound live in tests/kernel_oracles.py.

Kinds of check:
  * pointer attention (one key 60+ nats above all others) -> EVERY output
    row bit-equal to one V row, for six target maps that sit on the causal
    diagonal, on 64-key tile edges and on the 32-row wave edge, at every
    tail geometry (S % 256 == 128: dead upper waves; S % 128 == 64 for v1)
    and with a GQA ratio of 3;
  * future decoy (the first MASKED key would dominate) and random /
    staircase data -> fp64 softmax within (2^-8 + 2^-12) max|V|, row 0
    bit-equal to V[0]; the staircases walk defer-max through defer-defer-
    rescale, alternate, always-rescale and always-defer;
  * vt_from_qkv -> bit-equal to permute().contiguous() on every tail path.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_oracles as ko
from senweaver_amd import ops

HEAD_CONFIGS = [(1, 1, 1), (2, 4, 2), (1, 6, 2)]   # (B, H, Hk); ratio 3 last
S_LISTS = {
    "v1": [64, 128, 192, 320],
    "v2": [128, 256, 384],
    "v3": [128, 256, 384, 512, 640],
    "v5": [128, 256, 384, 512, 640],
}
KERNEL_S = [(kern, S) for kern, Ss in S_LISTS.items() for S in Ss]
RANDOM_S = {"v1": [192, 320], "v2": [384, 640], "v3": [384, 640], "v5": [384, 640]}
KERNEL_RANDOM_S = [(kern, S) for kern, Ss in RANDOM_S.items() for S in Ss]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_loaded(), "HIP extension failed to build/load"
    return torch.device("cuda:0")


@pytest.fixture
def gen():
    return torch.Generator().manual_seed(20241)


def _kernel(name):
    """The op under test as fn(q, k, vt, scale) -> O^T [B,H,D,S]."""
    ext = ops.hip_ext()
    if name == "v1":   # returns [B,H,S,D]
        return lambda q, k, vt, s: ext.attn_fwd(q, k, vt, s).transpose(-1, -2).contiguous()
    return {"v2": ext.attn_fwd_v2, "v3": ext.attn_fwd_v3, "v5": ext.attn_fwd_v5}[name]


def _ops_attn_fwd(q, k, vt, s):
    return ops.attn_fwd(q, k, None, s, vt=vt).transpose(-1, -2).contiguous()


# ---------------- 1. pointer attention: every row bit-exact ----------------
@pytest.mark.parametrize("tmap", ko.POINTER_MAPS)
@pytest.mark.parametrize("kern,S", KERNEL_S)
def test_pointer_bit_exact(dev, gen, kern, S, tmap):
    for B, H, Hk in HEAD_CONFIGS:
        ko.check_pointer(_kernel(kern), B, H, Hk, S, tmap, dev, gen)


# ---------------- 2. future decoy ----------------
@pytest.mark.parametrize("kern,S", KERNEL_S)
def test_future_decoy_is_masked(dev, gen, kern, S):
    ko.check_future_decoy(_kernel(kern), 2, 4, 2, S, dev, gen)


# ---------------- 3. random and staircase data against fp64 ----------------
@pytest.mark.parametrize("mode", ko.PREFILL_MODES)
@pytest.mark.parametrize("kern,S", KERNEL_RANDOM_S)
def test_prefill_vs_fp64(dev, gen, kern, S, mode):
    ko.check_prefill_random(_kernel(kern), mode, 1, 4, 2, S, dev, gen)


# ---------------- 5. dispatch boundary through the public ops ----------------
# ops.attn_fwd_t takes v5 when ceil(S/256) * B * H >= 512, else v2.
@pytest.mark.parametrize("tmap", ["diag", "random"])
@pytest.mark.parametrize("B,H,Hk", [(1, 512, 512),    # == 512: v5
                                    (1, 511, 511),    # v2
                                    (2, 256, 64)])    # v5, GQA 4, batch stride
@pytest.mark.parametrize("op", ["attn_fwd_t", "attn_fwd"])
def test_dispatch_boundary_pointer(dev, gen, op, B, H, Hk, tmap):
    fn = ops.attn_fwd_t if op == "attn_fwd_t" else _ops_attn_fwd
    ko.check_pointer(fn, B, H, Hk, 256, tmap, dev, gen)


@pytest.mark.parametrize("tmap", ["diag", "random"])
def test_ops_attn_fwd_v1_route(dev, gen, tmap):
    """S = 192 is no multiple of 128: ops.attn_fwd runs the 64-row kernel."""
    for B, H, Hk in HEAD_CONFIGS:
        ko.check_pointer(_ops_attn_fwd, B, H, Hk, 192, tmap, dev, gen)


def _bshd_view(t):
    """The same values as a permuted view of a [B,S,H,D] buffer."""
    view = t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    assert view.shape == t.shape and not view.is_contiguous()
    return view


@pytest.mark.parametrize("tmap", ["diag", "random"])
@pytest.mark.parametrize("op,B,H,Hk,S", [("attn_fwd_t", 2, 256, 64, 256),   # v5
                                         ("attn_fwd_t", 2, 4, 2, 256),      # v2
                                         ("attn_fwd", 2, 256, 64, 256),
                                         ("attn_fwd", 2, 4, 2, 192)])       # v1
def test_ops_accept_noncontiguous_q_k(dev, gen, op, B, H, Hk, S, tmap):
    """q and k as permuted [B,S,H,D] views, vt given, v=None."""
    fn = ops.attn_fwd_t if op == "attn_fwd_t" else _ops_attn_fwd
    ko.check_pointer(fn, B, H, Hk, S, tmap, dev, gen, prep=_bshd_view)


# ---------------- 6. binding checks ----------------
def _bindings():
    ext = ops.hip_ext()
    return {
        "attn_fwd": ext.attn_fwd,
        "attn_fwd_v2": ext.attn_fwd_v2,
        "attn_fwd_v3": ext.attn_fwd_v3,
        "attn_fwd_v5": ext.attn_fwd_v5,
    }


@pytest.mark.parametrize("name", ["attn_fwd", "attn_fwd_v2", "attn_fwd_v3",
                                  "attn_fwd_v5"])
def test_bindings_reject_mismatched_k_vt(dev, gen, name):
    """k's batch, sequence and head dimensions and vt's batch must match q.
    Only OVERSIZED operands are used, so a binding without the check would
    read in bounds (at the wrong rows) instead of raising."""
    fn = _bindings()[name]
    B, H, Hk, S, D = 1, 2, 2, 128, 128
    q = ko.rand_bf16(gen, B, H, S, D).to(dev)
    k = ko.rand_bf16(gen, B, Hk, S, D).to(dev)
    vt = ko.rand_bf16(gen, B, Hk, D, S).to(dev)
    scale = ko.PREFILL_SCALE
    fn(q, k, vt, scale)   # the matching shapes are accepted
    bad_k = {
        "S + 128 rows": ko.rand_bf16(gen, B, Hk, S + 128, D),
        "B + 1 batches": ko.rand_bf16(gen, B + 1, Hk, S, D),
        "2 D columns": ko.rand_bf16(gen, B, Hk, S, 2 * D),
    }
    for what, kk in bad_k.items():
        with pytest.raises(RuntimeError):
            fn(q, kk.to(dev), vt, scale)
            pytest.fail(f"{name} accepted k with {what}")
    with pytest.raises(RuntimeError):
        fn(q, k, ko.rand_bf16(gen, B + 1, Hk, D, S).to(dev), scale)
        pytest.fail(f"{name} accepted vt with B + 1 batches")
    torch.cuda.synchronize()


# ---------------- 7. vt_from_qkv tails ----------------
VT_HEADS = [(1, 1), (4, 2), (6, 2)]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [1, 7, 8, 31, 33, 100])
def test_vt_from_qkv_tails_bit_exact(dev, gen, S, D):
    """S below / across the 8-wide store vector and the 32-row tile; D = 64
    fills one 64-column block, D = 128 two."""
    for Hq, Hk in VT_HEADS:
        for B in (1, 2):
            ko.check_vt_from_qkv(ops.vt_from_qkv, B, S, Hq, Hk, D, dev, gen)


@pytest.mark.parametrize("S", [7, 33, 100])
def test_vt_from_qkv_wide_rows(dev, gen, S):
    """Rows longer than (Hq + 2 Hk) D.  The binding takes the row stride from
    qkv.size(1) and requires a contiguous tensor, so a wider row is passed
    as extra trailing columns (a multiple of 8: 16-byte loads); a strided
    VIEW is refused by the binding and copied by ops.vt_from_qkv."""
    ext = ops.hip_ext()
    for Hq, Hk in VT_HEADS:
        ko.check_vt_from_qkv(ext.vt_from_qkv, 2, S, Hq, Hk, 128, dev, gen, extra_cols=8)
        ko.check_vt_from_qkv(ops.vt_from_qkv, 2, S, Hq, Hk, 64, dev, gen, extra_cols=72)

    def through_view(fn):
        def run(qkv, Hq, Hk, D, B, S_):
            wide = torch.cat([qkv, torch.zeros_like(qkv[:, :16])], dim=1)
            view = wide[:, :qkv.shape[1]]
            assert not view.is_contiguous()
            return fn(view, Hq, Hk, D, B, S_)
        return run

    ko.check_vt_from_qkv(through_view(ops.vt_from_qkv), 2, S, 4, 2, 128, dev, gen)
    with pytest.raises(RuntimeError):
        ko.check_vt_from_qkv(through_view(ext.vt_from_qkv), 2, S, 4, 2, 128, dev, gen)
    with pytest.raises(RuntimeError):   # 16-byte loads need rows of 8 k elements
        ko.check_vt_from_qkv(ext.vt_from_qkv, 2, S, 4, 2, 128, dev, gen, extra_cols=3)
