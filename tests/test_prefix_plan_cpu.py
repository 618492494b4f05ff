"""Prefix-packed prefill on the CPU: the layout plan, and the index plumbing
of LlamaModel.prefill_packed / the scorer through the reference ops."""

import pytest
import torch

import prefix_pack_cases as pc
from senweaver_amd.engine.prefix_plan import (PrefixPlan, adjacent_lcp,
                                              plan_from_lcp, plan_from_tokens)
from senweaver_amd.engine.scorer import LlamaBackend
from senweaver_amd.models.config import get_config
from senweaver_amd.models.llama import LlamaModel
from senweaver_amd.ops import reference as ref


def _check_bijection(plan: PrefixPlan):
    """Stored (b, s) -> packed row is a bijection onto [0, Tp), in packed-row
    order; a member's prefix maps into its leader's rows."""
    stored = plan.stored_tokens()
    assert len(stored) == plan.Tp
    assert [plan.packed_row(b, s) for b, s in stored] == list(range(plan.Tp))
    for b in range(plan.B):
        o = plan.owner[b]
        assert plan.owner[o] == o and plan.skip[o] == 0 and o <= b
        for s in (0, plan.skip[b] - 1):
            if 0 <= s < plan.skip[b]:
                assert plan.packed_row(b, s) == plan.packed_row(o, s)
    assert plan.Tp % plan.G == 0 or plan.S % plan.G != 0


def test_no_sharing_is_identity():
    plan = plan_from_lcp([0, 0, 3, 0], 256)
    assert plan.is_identity and plan.Tp == 4 * 256
    assert plan.owner == (0, 1, 2, 3) and plan.skip == (0, 0, 0, 0)
    assert plan.base == (0, 256, 512, 768)
    _check_bijection(plan)


def test_bench_shape():
    plan = plan_from_lcp([0, 500, 500, 500], 2048)
    assert plan.skip == (0, 448, 448, 448)
    assert plan.owner == (0, 0, 0, 0)
    assert plan.Tp == 6848
    assert plan.base == (0, 2048 - 448, 2048 + 1600 - 448, 2048 + 3200 - 448)
    _check_bijection(plan)
    assert plan_from_lcp([0, 500, 500, 500], 2048, G=128).Tp == 7040


def test_two_groups_in_a_microbatch_of_8():
    plan = plan_from_lcp([0, 200, 200, 200, 5, 130, 130, 130], 512)
    assert plan.owner == (0, 0, 0, 0, 4, 4, 4, 4)
    assert plan.skip == (0, 192, 192, 192, 0, 128, 128, 128)
    assert plan.Tp == 2 * 512 + 3 * 320 + 3 * 384
    _check_bijection(plan)


def test_group_of_three_then_singleton():
    plan = plan_from_lcp([0, 100, 100, 63], 256)
    assert plan.owner == (0, 0, 0, 3)
    assert plan.skip == (0, 64, 64, 0)
    assert plan.base[3] == 256 + 192 + 192 and plan.Tp == 256 * 2 + 192 * 2
    _check_bijection(plan)


def test_lcp_shrinking_along_a_group():
    # row 1 shares 200 with the leader; row 2 shares 250 with row 1 but only
    # 200 with the leader (chain minimum); row 3 shares 130 with row 2
    plan = plan_from_lcp([0, 200, 250, 130], 512)
    assert plan.owner == (0, 0, 0, 0)
    assert plan.skip == (0, 192, 192, 128)
    _check_bijection(plan)
    # the chain minimum never exceeds the true prefix with the leader
    rows = [[1] * 300, [1] * 200 + [2] * 100, [1] * 200 + [2] * 50 + [3] * 50,
            [1] * 130 + [4] * 170]
    assert adjacent_lcp(rows) == [0, 200, 250, 130]


def test_identical_rows_cap_skip_at_S_minus_G():
    plan = plan_from_lcp([0, 256, 256], 256)
    assert plan.skip == (0, 192, 192) and plan.Tp == 256 + 64 + 64
    _check_bijection(plan)


def test_lcp_below_granule_does_not_pack():
    plan = plan_from_lcp([0, 63, 63, 63], 256)
    assert plan.is_identity
    assert plan_from_lcp([0, 64, 63, 127], 256).skip == (0, 64, 0, 64)


def test_plan_from_tokens_and_device_map():
    tokens = pc.shared_prefix_tokens(4, 256, 200, 512)
    plan = plan_from_tokens(tokens.tolist())
    assert plan.skip == (0, 192, 192, 192) and plan.Tp == 256 + 3 * 64
    _check_bijection(plan)
    skip, base, owner = (torch.tensor(x, dtype=torch.int32)
                         for x in (plan.skip, plan.base, plan.owner))
    src = ref.packed_src_rows_ref(plan.B, plan.S, skip, base, owner)
    exp = [[plan.packed_row(b, s) for s in range(plan.S)] for b in range(plan.B)]
    assert src.tolist() == exp


@pytest.mark.parametrize("name", ["tiny-debug", "tiny-moe"])
def test_prefill_packed_matches_prefill_cpu(name):
    cfg = get_config(name)
    model = LlamaModel(cfg, device="cpu", seed=0)
    tokens = pc.shared_prefix_tokens(4, 256, 200, cfg.vocab_size)
    plan = pc.check_prefill_packed(model, tokens)
    assert plan.skip == (0, 192, 192, 192)


def test_scorer_prefix_pack_switch_cpu():
    tokens = pc.shared_prefix_tokens(4, 256, 200, 512)
    mask = torch.zeros(4, 256, dtype=torch.bool)
    mask[:, 150:180] = True     # scored inside the shared prefix ...
    mask[:, 190:230] = True     # ... across the skip edge, and past it
    mask[2, 255] = True

    def make(pack):
        return LlamaBackend("tiny-debug", device="cpu", seed=0, max_seq=256,
                            micro_batch=4, prefix_pack=pack)

    pc.check_scorer(make, tokens, mask)
