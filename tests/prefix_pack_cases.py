"""Shared pieces of the prefix-packed prefill tests (CPU and GPU).

Model-level comparisons are not bit-equal: the packed path runs its GEMMs at
M = Tp instead of B*S, and a different M can select a different library GEMM
(another K-split, another summation order).  The tolerance is therefore
MEASURED on the unchanged path inside each test: ``prefill`` on the same rows
at B=4 and again row by row at B=1 differ by exactly that effect.  Packed
against unpacked must stay within 2x of it (two GEMM shapes differ from the
B=4 run instead of one), in max abs and in max relative difference.

Relative difference is |a - b| / max(|b|, rms(b)): the hidden states are
RMS-normalised, and an element that happens to sit near zero carries the
absolute error of its row, not a relative one, so the denominator is floored
at the tensor's RMS.
"""

import torch

from senweaver_amd.engine.prefix_plan import plan_from_tokens


def shared_prefix_tokens(B, S, prefix, vocab, seed=7, lo=3):
    """[B, S] int64 tokens whose rows share exactly the first ``prefix``."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, vocab, (B, S), generator=g)
    t[:, :prefix] = t[0, :prefix]
    for b in range(1, B):      # make the first differing token differ
        t[b, prefix] = lo + (int(t[0, prefix]) - lo + b) % (vocab - lo)
    return t


def diffs(a: torch.Tensor, b: torch.Tensor):
    """(max abs, max relative) difference of a against the reference b."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    d = (a - b).abs()
    floor = b.pow(2).mean().sqrt()
    return float(d.max()), float((d / b.abs().clamp(min=float(floor))).max())


def assert_within_noise(what, got, ref, noise_a, noise_b, factor=2.0):
    """got vs ref within ``factor`` x the measured (noise_a vs noise_b)."""
    n_abs, n_rel = diffs(noise_a, noise_b)
    g_abs, g_rel = diffs(got, ref)
    print(f"{what}: noise abs {n_abs:.3e} rel {n_rel:.3e} | "
          f"packed-vs-unpacked abs {g_abs:.3e} rel {g_rel:.3e}")
    assert g_abs <= factor * n_abs, f"{what}: abs {g_abs:.3e} > {factor} x {n_abs:.3e}"
    assert g_rel <= factor * n_rel, f"{what}: rel {g_rel:.3e} > {factor} x {n_rel:.3e}"


def check_prefill_packed(model, tokens):
    """prefill_packed == rows of prefill at the mapped indices, within 2x the
    B=4-vs-B=1 noise of prefill itself.  Returns the plan."""
    B, S = tokens.shape
    plan = plan_from_tokens(tokens.tolist())
    assert not plan.is_identity
    dev_tokens = tokens.to(model.device)
    full = model.prefill(dev_tokens).reshape(B * S, -1)
    single = torch.cat([model.prefill(dev_tokens[b:b + 1]) for b in range(B)],
                       dim=1).reshape(B * S, -1)
    packed = model.prefill_packed(dev_tokens, plan)
    assert tuple(packed.shape) == (plan.Tp, full.shape[1])
    idx = torch.tensor([b * S + s for b, s in plan.stored_tokens()])
    assert_within_noise(f"prefill_packed {model.config.name}",
                        packed, full.cpu()[idx], single, full)
    return plan


def check_scorer(make_backend, tokens, mask):
    """score_token_batch with prefix_pack on vs off, within 2x the noise of
    the unpacked scorer (B=4 vs row by row)."""
    on = make_backend(True)
    off = make_backend(False)
    assert on.prefix_pack and not off.prefix_pack
    dt, dm = tokens.to(off.device), mask.to(off.device)
    ref = off.score_token_batch(dt, dm)
    single = torch.cat([off.score_token_batch(dt[b:b + 1], dm[b:b + 1])
                        for b in range(tokens.shape[0])])
    calls = []
    inner = on.model.prefill_packed
    on.model.prefill_packed = lambda t, p: (calls.append(p), inner(t, p))[1]
    got = on.score_token_batch(dt, dm)
    assert len(calls) == 1 and not calls[0].is_identity, "packed path not taken"
    assert_within_noise("scorer", got, ref, single, ref)
