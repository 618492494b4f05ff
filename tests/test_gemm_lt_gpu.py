"""The direct hipBLASLt binding and its per-shape tuner (csrc/gemm_lt.hip)
against the fp64 oracles in tests/kernel_oracles.py.

Every candidate the tuner would time is a different kernel with its own
summation order, so each must stay within the order-independent bound
2^-8 |ref| + K 2^-24 (|a|.|b|^T) on random data and be bit-exact on small
integers, where every fp32 partial sum is exact.  Shapes are small: M from
just above the GEMV threshold (17) through non-multiples of any tile, N 256
and 384 (not a multiple of 256), K of one and several k-steps.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_oracles as ko
from senweaver_amd import ops

MS = [17, 64, 200, 448]
MAX_CANDS = 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.extension_loaded(), "HIP extension failed to build/load"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext(dev):
    return ops.hip_ext()


@pytest.fixture
def gen():
    return torch.Generator().manual_seed(7100)


def _int_w(gen, N, K):
    return torch.randint(-4, 5, (N, K), generator=gen).to(ko.BF16)


def _strided(a, dev):
    """a as a column slice of a wider buffer (row stride K + 64)."""
    M, K = a.shape
    wide = torch.zeros(M, K + 64, dtype=a.dtype)
    wide[:, 32:32 + K] = a
    v = wide.to(dev)[:, 32:32 + K]
    assert v.stride() == (K + 64, 1)
    return v


def _transposed(a, dev):
    """a as the transposed view of a contiguous [K, M] tensor."""
    v = a.t().contiguous().to(dev).t()
    assert v.stride() == (1, a.shape[0]) and v.shape == a.shape
    return v


@pytest.mark.parametrize("K", [128, 512])
@pytest.mark.parametrize("N", [256, 384])
def test_every_candidate_random_and_integer(dev, ext, gen, N, K):
    wr, wi = ko.rand_bf16(gen, N, K), _int_w(gen, N, K)
    wr_d, wi_d = wr.to(dev), wi.to(dev)
    for M in MS:
        xr, xi = ko.rand_bf16(gen, M, K), ko.int_x(gen, M, K)
        ref = ko.gemv_ref64(xr, wr)
        bound = ko.gemv_bound(ref, ko.gemv_abs_dot(xr, wr), K)
        assert float(ko.gemv_abs_dot(xi, wi).max()) < 2 ** 24
        exact = ko.exact_bf16(ko.gemv_ref64(xi, wi))
        xr_d, xi_d = xr.to(dev), xi.to(dev)
        n = ext.gemm_lt_candidates(xr_d, wr_d)
        assert n >= 1, f"no hipBLASLt candidate for M={M} N={N} K={K}"
        for i in range(min(n, MAX_CANDS)):
            what = f"cand {i}/{n} M={M} N={N} K={K}"
            ko.assert_within(ext.gemm_lt_run(xr_d, wr_d, i), ref, bound, what + " random")
            ko.assert_bits_equal(ext.gemm_lt_run(xi_d, wi_d, i), exact, what + " integer")


@pytest.mark.parametrize("view", [_strided, _transposed])
def test_strided_and_transposed_a(dev, ext, gen, view):
    N, K = 384, 512
    wr, wi = ko.rand_bf16(gen, N, K), _int_w(gen, N, K)
    wr_d, wi_d = wr.to(dev), wi.to(dev)
    for M in MS:
        xr, xi = ko.rand_bf16(gen, M, K), ko.int_x(gen, M, K)
        ref = ko.gemv_ref64(xr, wr)
        bound = ko.gemv_bound(ref, ko.gemv_abs_dot(xr, wr), K)
        contiguous = ext.gemm_lt(xi.to(dev), wi_d)
        ko.assert_bits_equal(contiguous, ko.exact_bf16(ko.gemv_ref64(xi, wi)), f"M={M} contiguous")
        xr_v, xi_v = view(xr, dev), view(xi, dev)
        n = ext.gemm_lt_candidates(xr_v, wr_d)
        assert n >= 1, f"no hipBLASLt candidate for {view.__name__} M={M}"
        for i in range(min(n, MAX_CANDS)):
            what = f"{view.__name__} cand {i}/{n} M={M}"
            ko.assert_within(ext.gemm_lt_run(xr_v, wr_d, i), ref, bound, what + " random")
            ko.assert_bits_equal(ext.gemm_lt_run(xi_v, wi_d, i), contiguous, what + " integer")
        ko.assert_bits_equal(ext.gemm_lt(xi_v, wi_d), contiguous, f"{view.__name__} M={M} gemm_lt")


def test_out_rows_pads_the_problem_not_the_result(dev, ext, gen):
    M, rows, N, K = 200, 256, 384, 512
    wi = _int_w(gen, N, K).to(dev)
    buf = torch.zeros(rows, K, dtype=ko.BF16)
    buf[:M] = ko.int_x(gen, M, K)
    buf = buf.to(dev)
    plain = ext.gemm_lt(buf[:M], wi)
    padded = ext.gemm_lt(buf[:M], wi, rows)
    assert tuple(padded.shape) == (M, N)
    ko.assert_bits_equal(padded, plain, "out_rows=256 against the unpadded call")
    with pytest.raises(RuntimeError):   # rows past A's storage are refused
        ext.gemm_lt(buf[:M], wi, rows + 1)


def test_tuned_choice_is_cached_and_reproducible(dev, ext, gen):
    M, N, K = 448, 384, 512
    a, b = ko.rand_bf16(gen, M, K).to(dev), ko.rand_bf16(gen, N, K).to(dev)
    before = ext.gemm_lt_stats()["tunes"]
    r1 = ext.gemm_lt_tune(a, b, 0, [b], True)   # forced: far below the size floor
    assert r1["status"] in ("tuned", "cached")
    mid = ext.gemm_lt_stats()["tunes"]
    assert mid - before == (1 if r1["status"] == "tuned" else 0)
    r2 = ext.gemm_lt_tune(a, b, 0, [b], True)
    assert r2["status"] == "cached" and r2["chosen"] == r1["chosen"]
    assert ext.gemm_lt_stats()["tunes"] == mid, "a cached key was tuned again"
    c1, c2 = ext.gemm_lt(a, b), ext.gemm_lt(a, b)
    ko.assert_bits_equal(c1, c2, "the chosen algorithm, run twice")
    ref = ko.gemv_ref64(a, b)
    ko.assert_within(c1, ref, ko.gemv_bound(ref, ko.gemv_abs_dot(a, b), K), "the chosen algorithm")
    for row in r1["candidates"]:
        assert row["status"] != "not reproducible" or row["cand"] != r1["chosen"]
    # an unforced call at this size is not worth tuning
    small = ext.gemm_lt_tune(a[:64], b, 0, [b], False)
    assert small["status"] == "small"


def test_two_streams_at_once(dev, ext, gen):
    """Each stream has its own workspace: the same GEMM issued on two streams
    concurrently equals its serial result."""
    M, N, K = 448, 384, 512
    a, b = ko.rand_bf16(gen, M, K).to(dev), ko.rand_bf16(gen, N, K).to(dev)
    serial = ext.gemm_lt(a, b)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(8):
        for s in (s1, s2):
            with torch.cuda.stream(s):
                outs.append(ext.gemm_lt(a, b))
    torch.cuda.synchronize()
    for i, c in enumerate(outs):
        ko.assert_bits_equal(c, serial, f"stream {i % 2} call {i // 2}")
    assert ext.gemm_lt_stats()["workspaces"] >= 2


def test_tune_off_is_torch_matmul(dev, ext, gen, monkeypatch):
    M, N, K = 2048, 4096, 6400   # above the tuner's size floor
    a, b = ko.rand_bf16(gen, M, K).to(dev), ko.rand_bf16(gen, N, K).to(dev)
    monkeypatch.setattr(ops, "_GEMM_TUNE", False)
    before = ext.gemm_lt_stats()["tunes"]
    ko.assert_bits_equal(ops.gemm_bt(a, b), a @ b.t(), "SENWEAVER_GEMM_TUNE=0")
    assert ext.gemm_lt_stats()["tunes"] == before


def test_ops_route_tunes_large_gemms_once(dev, ext, gen):
    """ops.gemm_bt sends a large bf16 GEMM through the tuner (integer data:
    any solution must reproduce torch.matmul bit for bit)."""
    M, N, K = 2048, 4096, 6400
    a = ko.int_x(gen, M, K).to(dev)
    b = _int_w(gen, N, K).to(dev)
    expect = a @ b.t()
    got = ops.gemm_bt(a, b)
    assert ops.gemm_lt_route(a, b), "a 1e11-flop bf16 GEMM is on the tuned route"
    tunes = ext.gemm_lt_stats()["tunes"]
    ko.assert_bits_equal(got, expect, "tuned route, integer data")
    ko.assert_bits_equal(ops.gemm_bt(a, b), expect, "second call")
    assert ext.gemm_lt_stats()["tunes"] == tunes
    small = a[:64]
    assert not ops.gemm_lt_route(small, b), "small GEMMs keep the torch.matmul route"
