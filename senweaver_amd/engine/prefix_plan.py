"""Layout plan for prefix-packed prefill.

Attention is causal, so rows of a microbatch that begin with the same tokens
have identical hidden states over that prefix at every layer.  The scorer's
microbatches are built candidate-major ([BOS, SYSTEM, candidate prompt,
rollout...] for every rollout of one candidate), so consecutive rows share
the whole candidate prompt.  A plan stores such a prefix once:

* rows are grouped greedily over CONSECUTIVE rows; the first row of a group
  is its *leader* (``owner[b] == b``, ``skip[b] == 0``) and stores all S rows;
* every other row of the group (a *member*) stores only ``s >= skip[b]``,
  where ``skip[b]`` is its common-prefix length with the leader rounded DOWN
  to the granule G and capped at ``S - G``;
* the packed row of token ``(b, s)`` is::

      s >= skip[b]:  base[b] + s
      s <  skip[b]:  base[owner[b]] + s

``Tp = sum(S - skip[b])`` rows go through every row-wise op (GEMMs, norms,
SwiGLU) instead of ``B * S``; only rope_scatter, the attention kernel's V
staging (the V^T transpose where the v5 kernel does not run) and its epilogue
translate between packed rows and the [B, H, S, D] attention layouts
(ops/csrc/README.md).  Pure Python: no torch import, the
plan is a handful of ints per row.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence, Tuple

GRANULE = 64  # two 32-row attention waves; S % 128 == 0 keeps Tp % 64 == 0


@dataclass(frozen=True)
class PrefixPlan:
    B: int
    S: int
    G: int
    owner: Tuple[int, ...]
    skip: Tuple[int, ...]
    base: Tuple[int, ...]
    Tp: int

    @property
    def is_identity(self) -> bool:
        """No row shares anything: the packed layout IS the [B*S] layout."""
        return self.Tp == self.B * self.S

    def packed_row(self, b: int, s: int) -> int:
        """Packed row holding token (b, s)."""
        if s < self.skip[b]:
            return self.base[self.owner[b]] + s
        return self.base[b] + s

    def stored_tokens(self) -> List[Tuple[int, int]]:
        """(b, s) of every packed row, in packed-row order."""
        out = []
        for b in range(self.B):
            out.extend((b, s) for s in range(self.skip[b], self.S))
        return out


def plan_from_skips(owner: Sequence[int], skip: Sequence[int], S: int,
                    G: int = GRANULE) -> PrefixPlan:
    """Lay out rows whose leader and skip are already decided."""
    base, nxt = [], 0
    for sk in skip:
        base.append(nxt - sk)
        nxt += S - sk
    return PrefixPlan(len(skip), S, G, tuple(owner), tuple(skip), tuple(base), nxt)


def plan_from_lcp(lcp_prev: Sequence[int], S: int, G: int = GRANULE) -> PrefixPlan:
    """Plan for B rows of length S.

    ``lcp_prev[b]`` is the common-prefix length of row b with row b-1
    (``lcp_prev[0]`` is ignored).  The prefix a row shares with its leader is
    at least the minimum of the adjacent values since the leader, which is
    what is used: never more than the true value, so sharing stays exact.
    """
    B = len(lcp_prev)
    owner, skip = [], []
    leader = 0
    chain = 0        # min adjacent lcp since the leader
    for b in range(B):
        shared = 0
        if b > 0 and S > G:
            chain = min(chain, int(lcp_prev[b]))
            shared = min((chain // G) * G, S - G)
        if shared >= G:
            owner.append(leader)
            skip.append(shared)
        else:
            leader, chain = b, S
            owner.append(b)
            skip.append(0)
    return plan_from_skips(owner, skip, S, G)


def adjacent_lcp(rows: Sequence[Sequence[int]]) -> List[int]:
    """Host version of the device lcp: common prefix of each row with the
    previous one (entry 0 is 0)."""
    out = [0]
    for prev, cur in zip(rows, rows[1:]):
        n = 0
        for a, c in zip(prev, cur):
            if a != c:
                break
            n += 1
        out.append(n)
    return out


def plan_from_tokens(rows: Sequence[Sequence[int]], G: int = GRANULE) -> PrefixPlan:
    S = len(rows[0]) if len(rows) else 0
    return plan_from_lcp(adjacent_lcp(rows), S, G)
