"""Model-level exactness on the GPU: every forward path of LlamaModel and the
scorer against the independent fp64 oracle of tests/model_oracle.py.

Every case compares per token row: || device - exact || <= 2 || rounded -
exact ||, both sides of the bound from the oracle alone (model_oracle.py's
docstring).  The configurations are built here, not taken from presets:
head_dim 128, 2 layers, vocab 512, rep 3 or 4 GQA, and weights rescaled so
that wiring errors show (model_oracle.rescale_weights_).  The same drivers
run on the model's CPU path in test_model_oracle_cpu.py, where the premises
and the mutants are checked as well.

Each test prints its worst err / noise ratio (KERNELS.md lists them).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import model_oracle as mo
from senweaver_amd import ops

QUANTS = ["bf16", "fp8", "mxfp8"]
REAL_LENS, FORCED = mo.REAL_LENS, mo.FORCED
_MODELS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_loaded(), "HIP extension failed to build/load"
    return "cuda:0"


class _ExtSpy:
    """The HIP extension, with the name of every kernel binding fetched."""

    def __init__(self, ext):
        self._ext, self.called = ext, set()

    def __getattr__(self, name):
        self.called.add(name)
        return getattr(self._ext, name)


@pytest.fixture
def ext_calls(dev, monkeypatch):
    """Set of extension bindings the test's forward went through: a case
    that names a kernel asserts that this kernel ran."""
    spy = _ExtSpy(ops.hip_ext())
    monkeypatch.setattr(ops, "hip_ext", lambda: spy)
    return spy.called


def model_of(dev, key, cfg, quant="bf16"):
    if (key, quant) not in _MODELS:
        _MODELS[(key, quant)] = mo.build_model(cfg, quant, dev)
    return _MODELS[(key, quant)]


def small(dev, quant="bf16"):
    return model_of(dev, "small", mo.cfg_small(), quant)


def gemv(dev, quant="bf16"):
    return model_of(dev, "gemv", mo.cfg_gemv(), quant)


def moe(dev, quant="bf16"):
    return model_of(dev, "moe", mo.cfg_moe(), quant)


# ---- prefill routes ----
@pytest.mark.parametrize("S", [64, 128, 192])
@pytest.mark.parametrize("quant", QUANTS)
def test_prefill_small(dev, quant, S):
    """S=128: attn_fwd_t, bf16 with o_proj off the O^T view, the quantized
    models through the permute; S=64 / 192: the v1 kernel."""
    mo.run_prefill(small(dev, quant), mo.dense_tokens(2, S), f"prefill small {quant} S={S}")


def test_prefill_tied_embeddings(dev):
    m = model_of(dev, "tied", mo.cfg_small(tie=True))
    assert m.lm_head is m.embed
    mo.run_prefill(m, mo.dense_tokens(2, 128), "prefill small tied")


def test_prefill_gemv_config(dev):
    mo.run_prefill(gemv(dev), mo.dense_tokens(2, 128), "prefill gemv bf16 S=128")


def test_prefill_wide_grid_s128(dev, ext_calls):
    """1 layer, 8 heads, B=64, S=128: ceil(S/256) B H = 512 blocks (below
    S = 256 ops.attn_fwd_t stays on v2 whatever the grid)."""
    m = model_of(dev, "wide128", mo.cfg_small(layers=1, heads=8))
    mo.run_prefill(m, mo.dense_tokens(64, 128), "prefill B=64 S=128 H=8")
    assert "attn_fwd_v2" in ext_calls and "attn_fwd_v5" not in ext_calls


def test_prefill_v5_kernel(dev, ext_calls):
    """ops.attn_fwd_t takes v5 only from S = 256 on: 1 layer, 16 heads, B=32,
    S=256, again 512 blocks, is the smallest shape on the v5 side."""
    m = model_of(dev, "v5", mo.cfg_small(layers=1, heads=16, kv_heads=4))
    mo.run_prefill(m, mo.dense_tokens(32, 256), "prefill B=32 S=256 H=16 (v5)")
    assert "attn_fwd_v5" in ext_calls and "attn_fwd_v2" not in ext_calls


# ---- prefill into the cache, decode, extend ----
def test_prefill_into_cache(dev):
    mo.run_prefill_cache(gemv(dev), mo.dense_tokens(2, 128), REAL_LENS,
                         "prefill+cache gemv")


@pytest.mark.parametrize("mode", ["eager", "graph"])
@pytest.mark.parametrize("quant", QUANTS)
def test_decode_batch2(dev, quant, mode):
    """decode_step and DecodeGraph.step_batch, batch 2 of unequal lengths;
    the quantized models through gemv_fp8w / gemv_mxfp8w and the quantized
    lm_head GEMV."""
    mo.run_decode(gemv(dev, quant), mo.dense_tokens(2, 128), REAL_LENS, FORCED,
                  mode, f"decode {mode} gemv {quant} B=2")


@pytest.mark.parametrize("quant", QUANTS)
def test_decode_single_graph(dev, quant, ext_calls):
    """DecodeGraph.step at B=1: the streaming GEMV."""
    mo.run_decode(gemv(dev, quant), mo.dense_tokens(2, 128)[1:], REAL_LENS[1:],
                  FORCED[1:], "graph1", f"decode graph gemv {quant} B=1")
    gemv_binding = {"bf16": "gemm_bt", "fp8": "gemv_bt_fp8w", "mxfp8": "gemv_bt_mxfp8w"}
    assert gemv_binding[quant] in ext_calls and "paged_decode_attn" in ext_calls


def test_decode_single_graph_normfuse(dev, ext_calls, monkeypatch):
    """SENWEAVER_DECODE_NORMFUSE=1: gemv_norm_bt in place of norm + GEMV
    before the qkv and the gate|up projection, same bound."""
    monkeypatch.setenv("SENWEAVER_DECODE_NORMFUSE", "1")
    mo.run_decode(gemv(dev), mo.dense_tokens(2, 128)[1:], REAL_LENS[1:],
                  FORCED[1:], "graph1", "decode graph gemv bf16 B=1 NORMFUSE")
    assert "gemv_norm_bt" in ext_calls


def test_prefill_extend(dev):
    mo.run_extend(gemv(dev), mo.dense_tokens(1, 137, seed=13), 100, 37,
                  "prefill_extend gemv 100+37")


# ---- MoE ----
@pytest.mark.parametrize("T", [9, 130, 300])
@pytest.mark.parametrize("quant", QUANTS)
def test_moe_layer(dev, quant, T):
    """_moe_ffn called directly with constructed routing: the sync-free bf16
    path (device cumsum offsets, inv = argsort(order), moe_combine) and the
    padded dest / inv_pad / w_pad layout of the quantized one."""
    mo.run_moe_layer(moe(dev, quant), T, f"moe layer {quant} T={T}")


@pytest.mark.parametrize("quant", QUANTS)
def test_moe_model(dev, quant):
    mo.run_prefill(moe(dev, quant), mo.moe_tokens(quant), f"prefill moe {quant} S=64")


# ---- scorer ----
@pytest.mark.parametrize("micro_batch", [None, 2])
@pytest.mark.parametrize("prefix_pack", [True, False])
def test_scorer(dev, prefix_pack, micro_batch):
    """score_token_batch_device, and score_microbatches over two streams."""
    mo.run_scorer(small(dev), prefix_pack, micro_batch,
                  f"scorer pack={prefix_pack} micro_batch={micro_batch}")


def test_scorer_packed_kernels(dev, ext_calls):
    """S = 256: from here on prefill_packed runs the packed rope / V^T
    kernels on the GPU instead of handing the unpacked prefill's rows back."""
    mo.run_scorer(small(dev), True, None, "scorer pack=True S=256", S=256)
    assert {"rope_scatter_qkv_packed", "vt_from_qkv_packed"} <= ext_calls
