"""LlamaModel.prefill_extend on the CPU (reference ops) against the full
prefill, judged by the measured decode-path noise
(tests/prefill_extend_cases.py)."""

import pytest
import torch

import prefill_extend_cases as pe
from senweaver_amd.models.config import get_config
from senweaver_amd.models.llama import LlamaModel


@pytest.fixture(scope="module")
def model():
    return LlamaModel(get_config("tiny-debug"), device=torch.device("cpu"), seed=0)


@pytest.fixture(scope="module")
def ref(model):
    with torch.no_grad():
        return pe.Reference(model)


@pytest.mark.parametrize("hist,n,Sq", [(128, 64, 64), (100, 37, 64)])
@torch.no_grad()
def test_prefill_extend_matches_prefill_cpu(model, ref, hist, n, Sq):
    pe.check_extend(model, ref, hist, n, Sq)


@torch.no_grad()
def test_prefill_extend_rejects_bad_lengths(model, ref):
    cache, seq = pe.prefill_history(model, ref.row, 16)
    tokens = torch.zeros(1, 64, dtype=torch.long)
    for bad in (0, 65):
        with pytest.raises(ValueError):
            model.prefill_extend(tokens, cache, [seq], [bad])
    assert cache.seq_lens[seq] == 16
