"""Exactness tests for the paged-context prefill attention kernel
(paged_prefill_attention.hip) on the GPU.  Builders and check drivers live in
tests/paged_prefill_cases.py, oracles and bounds in tests/kernel_oracles.py.

Kinds of check, each over the (ctx, q_len) edge list of the cases module:
  * pointer attention -> every real row bit-equal to one V row;
  * future decoy (row i's strongest key is new token i+1, present in the
    cache) and random data -> fp64 softmax within (2^-8 + 2^-12) max|V|;
  * pad rows and cache slots at positions >= ctx at the largest finite bf16
    -> not one output bit changes, pad rows are +0;
  * q_len == 1 against the decode kernel, each within its own bound;
  * the binding's argument checks.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_oracles as ko
import paged_prefill_cases as pp
from senweaver_amd import ops


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_loaded(), "HIP extension failed to build/load"
    return torch.device("cuda:0")


@pytest.fixture
def gen():
    return torch.Generator().manual_seed(20251)


def _fn():
    return ops.hip_ext().paged_prefill_attn


def test_scatter_construction_agrees_with_decode_oracle(gen):
    pp.check_scatter_agrees(gen)


# ---------------- 1. pointer attention: every real row bit-exact ----------
@pytest.mark.parametrize("tmap", ko.POINTER_MAPS)
@pytest.mark.parametrize("ctx,q_len", pp.CASES)
def test_pointer_bit_exact(dev, gen, ctx, q_len, tmap):
    pp.check_pointer(_fn(), dev, gen, ctx, q_len, tmap)


# ---------------- 2. future decoy: later new keys are present -------------
@pytest.mark.parametrize("ctx,q_len", pp.CASES)
def test_future_decoy_is_masked(dev, gen, ctx, q_len):
    pp.check_future_decoy(_fn(), dev, gen, ctx, q_len)


# ---------------- 3. random data, B = 2, mixed geometry --------------------
@pytest.mark.parametrize("H,Hk", [(H, Hk) for _, H, Hk in pp.HEAD_CONFIGS])
@pytest.mark.parametrize("geoms", pp.RANDOM_PAIRS)
def test_random_vs_fp64(dev, gen, geoms, H, Hk):
    pp.check_random(_fn(), dev, gen, list(geoms), H, Hk)


# ---------------- 4. pad rows and stale slots -------------------------------
@pytest.mark.parametrize("geoms", pp.RANDOM_PAIRS)
def test_pad_rows_and_stale_slots_change_nothing(dev, gen, geoms):
    pp.check_pad_and_stale(_fn(), dev, gen, list(geoms), 4, 2)


# ---------------- 5. q_len == 1 against the decode kernel -------------------
@pytest.mark.parametrize("H,Hk", [(H, Hk) for _, H, Hk in pp.HEAD_CONFIGS])
def test_agrees_with_decode_kernel(dev, gen, H, Hk):
    ctxs = [100, 333]
    c = ko.make_paged_case(gen, ctxs, H, Hk)
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    ref = ko.paged_decode_attn_ref64(c["q"], c["kcache"], c["vcache"],
                                     c["block_table"], c["ctx_lens"], c["scale"])
    dec = ops.paged_decode_attn(d["q"], d["kcache"], d["vcache"], d["block_table"],
                                d["ctx_lens"], c["scale"])
    pre = _fn()(d["q"].unsqueeze(1).contiguous(), d["kcache"], d["vcache"],
                d["block_table"], d["ctx_lens"], torch.ones_like(d["ctx_lens"]),
                c["scale"])
    what = f"q_len=1 H={H} Hk={Hk}"
    ko.assert_within(dec, ref, torch.tensor(ko.attn_bound(c["vcache"]), dtype=torch.float64),
                     what + " decode kernel")
    ko.assert_within(pre[:, 0], ref, torch.tensor(ko.prefill_bound(c["vcache"]),
                                                  dtype=torch.float64),
                     what + " prefill kernel")


# ---------------- 6. binding checks ------------------------------------------
def test_binding_checks(dev, gen):
    c = pp.make_random_case(gen, [(80, 16), (64, 64)], 4, 2)
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32, device=dev)
    good = dict(q=c["q"].to(dev), kc=c["kcache"].to(dev), vc=c["vcache"].to(dev),
                bt=c["block_table"].to(dev), ctx=i32(c["ctxs"]), ql=i32(c["qlens"]))

    def run(**over):
        a = dict(good, **over)
        return _fn()(a["q"], a["kc"], a["vc"], a["bt"], a["ctx"], a["ql"], c["scale"])

    assert tuple(run().shape) == tuple(good["q"].shape)
    P, _, Hk, D = good["kc"].shape
    bad = {
        "q dtype": dict(q=good["q"].half()),
        "cache dtype": dict(kc=good["kc"].float()),
        "q not contiguous": dict(q=good["q"].transpose(1, 2)),
        "D != 128": dict(q=good["q"][..., :64].contiguous(),
                         kc=good["kc"][..., :64].contiguous(),
                         vc=good["vc"][..., :64].contiguous()),
        "page size != 16": dict(kc=good["kc"].view(P * 2, 8, Hk, D),
                                vc=good["vc"].view(P * 2, 8, Hk, D)),
        "int64 block table": dict(bt=good["bt"].long()),
        "int64 ctx_lens": dict(ctx=good["ctx"].long()),
        "int64 q_lens": dict(ql=good["ql"].long()),
        "B mismatch (table)": dict(bt=good["bt"][:1].contiguous()),
        "B mismatch (ctx_lens)": dict(ctx=i32([80])),
        "B mismatch (q_lens)": dict(ql=i32([16, 64, 1])),
        "Sq == 0": dict(q=good["q"][:, :0].contiguous()),
        "more than 2048 pages per row": dict(
            bt=torch.full((2, 2049), -1, dtype=torch.int32, device=dev)),
    }
    for name, over in bad.items():
        with pytest.raises(RuntimeError):
            run(**over)
            print(f"binding accepted: {name}")
