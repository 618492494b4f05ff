"""LlamaModel.prefill_extend on the GPU (rope_kv_append on the real rows,
paged_prefill_attn) against the full prefill, judged by the measured
decode-path noise (tests/prefill_extend_cases.py)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import prefill_extend_cases as pe
from senweaver_amd import ops
from senweaver_amd.models.config import get_config
from senweaver_amd.models.llama import LlamaModel


@pytest.fixture(scope="module")
def model():
    assert torch.cuda.is_available()
    assert ops.extension_loaded(), "HIP extension failed to build/load"
    return LlamaModel(get_config("tiny-debug"), device=torch.device("cuda:0"), seed=0)


@pytest.fixture(scope="module")
def ref(model):
    with torch.no_grad():
        return pe.Reference(model)


@pytest.mark.parametrize("hist,n,Sq", [(128, 64, 64), (100, 37, 64)])
@torch.no_grad()
def test_prefill_extend_matches_prefill_gpu(model, ref, hist, n, Sq):
    pe.check_extend(model, ref, hist, n, Sq)
