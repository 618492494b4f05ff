"""Without a GPU the GEMM dispatch stays on the fp32 reference and never
touches the HIP extension or the hipBLASLt tuner."""

import os
import subprocess
import sys

import torch

from senweaver_amd import ops
from senweaver_amd.ops import reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpu_gemm_bt_is_the_reference():
    g = torch.Generator().manual_seed(3)
    b = torch.randn(24, 64, generator=g).to(torch.bfloat16)
    for M in (1, 17, 40):
        a = torch.randn(M, 64, generator=g).to(torch.bfloat16)
        assert torch.equal(ops.gemm_bt(a, b), ref.gemm_bt_ref(a, b))
        assert torch.equal(ops.gemm_bt(a.t().contiguous().t(), b), ref.gemm_bt_ref(a, b))
    assert not ops.gemm_lt_route(a, b)


def test_cpu_o_proj_off_the_transposed_view():
    g = torch.Generator().manual_seed(4)
    ot = torch.randn(2, 32, 16, generator=g).to(torch.bfloat16)   # [B, K, S]
    w = torch.randn(8, 32, generator=g).to(torch.bfloat16)
    got = ops.gemm_bt_heads_t(ot, w)
    exp = torch.matmul(ot.transpose(1, 2), w.t()).reshape(32, 8)
    assert got.shape == (32, 8) and torch.equal(got, exp)


def test_importing_ops_does_not_load_the_extension():
    code = ("import sys; import senweaver_amd.ops as o; "
            "assert o._ext is None and o._ext_err is None; "
            "assert 'senweaver_amd_hip' not in sys.modules; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
